"""Happens-before from the operation log of tests/cpu_backend_streams.c (tests/test_streams.py).

The backend runs everything synchronously but logs, in issue order, every launch with its stream and every event_record,
stream_wait and stream_sync.  check() rebuilds the order a real device would be bound by:

  * program order on each stream;
  * a stream_wait is ordered after the LATEST EARLIER record of its event (none: the wait orders nothing, as in HIP);
  * a stream_sync drains its stream and holds the issuing rank's host: everything that rank issues later comes after it;
  * a flag wait (direct-store exchange) is ordered after the first earlier signal that stored a value >= its own into the
    same word -- the one edge that crosses ranks, which are threads sharing one log there.

and reports, for a call bracketed by two marks on the caller's stream S: a launch that is not ordered after the entry mark
(missing fork), a launch the exit mark is not ordered after (missing join), a stream_sync inside the call (host wait), and
two unordered launches of which one writes what the other reads or writes (hazard; only with access recording on).

  _stream_graph.py world <size> <cases.json> <out.json>   ranks as threads on the CPU backend, each on a caller stream in
                                                          async mode: the violations of every case (the edge-drop controls)
  _stream_graph.py gloo <cases.json> <outdir>             one gloo rank per process (RANK / WORLD_SIZE / MASTER_* set)
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

KIND = {"pass": 0, "conv": 1, "conv_oop": 2, "conv_sum": 3, "filt_fwd": 4, "filt_inv": 5, "pointwise": 6, "pointwise_oop": 7,
        "pointwise_sum": 8, "memcpy": 9, "zero": 10, "a2a": 11, "flag_signal": 12, "flag_wait": 13,
        "event_record": 20, "stream_wait": 21, "stream_sync": 22, "mark": 30}
NAME = {v: k for k, v in KIND.items()}
ENTRY, EXIT = 1, 2
_NO = np.zeros(0, dtype=np.uint64)


class Rec(C.Structure):
    """srec of cpu_backend_streams.c"""
    _fields_ = [("kind", C.c_int), ("rank", C.c_int), ("stream", C.c_ulonglong), ("event", C.c_ulonglong), ("value", C.c_ulonglong),
                ("n", C.c_int), ("direction", C.c_int), ("ncols", C.c_int), ("nb1", C.c_int), ("half", C.c_int),
                ("real_input", C.c_int), ("out_keep", C.c_int), ("same", C.c_int),
                ("r_off", C.c_longlong), ("r_len", C.c_longlong), ("w_off", C.c_longlong), ("w_len", C.c_longlong)]


class Op:
    """one line of the log; reads / writes: sorted unique granule addresses (launches, with access recording)"""

    def __init__(self, kind, stream, event=0, value=0, rank=0, reads=_NO, writes=_NO, **desc):
        self.kind = KIND[kind] if isinstance(kind, str) else kind
        self.stream, self.event, self.value, self.rank = stream, event, value, rank
        self.reads, self.writes, self.desc = reads, writes, desc

    @property
    def name(self):
        return NAME[self.kind]

    @property
    def launch(self):
        return self.kind < 20

    def __repr__(self):
        return f"{self.name}(rank {self.rank}, stream {self.stream:#x}, n {self.desc.get('n', 0)})"


def streams_cb_lib():
    """tests/libcpubackend_streams.so, shaped like cpu_world's backend library"""
    import subprocess
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/libcpubackend_streams.so"])
    L = C.CDLL(os.path.join(ROOT, "tests", "libcpubackend_streams.so"))
    L.cpu_backend_streams_table.restype = C.c_void_p
    L.cpu_backend_table = L.cpu_backend_streams_table
    L.cpu_backend_pass_count.restype = C.c_long
    L.cpu_backend_streams_new_stream.restype = C.c_void_p
    L.cpu_backend_streams_free_stream.argtypes = [C.c_void_p]
    L.cpu_backend_streams_mark.argtypes = [C.c_void_p, C.c_ulonglong]
    L.cpu_backend_streams_len.restype = C.c_long
    L.cpu_backend_streams_copy_log.argtypes = [C.c_void_p]
    L.cpu_backend_streams_copy_access.argtypes = [C.c_longlong, C.c_longlong, C.c_void_p]
    L.cpu_backend_set_peer_open.argtypes = [C.c_void_p]
    assert L.cpu_backend_streams_rec_bytes() == C.sizeof(Rec)
    return L


def read_log(CB):
    """the log since the last reset, as Ops"""
    n = CB.cpu_backend_streams_len()
    recs = (Rec * max(n, 1))()
    CB.cpu_backend_streams_copy_log(recs)

    def access(off, ln):
        if not ln:
            return _NO
        a = np.empty(ln, dtype=np.uint64)
        CB.cpu_backend_streams_copy_access(off, ln, a.ctypes.data)
        return np.unique(a)
    return [Op(r.kind, r.stream, r.event, r.value, r.rank, access(r.r_off, r.r_len), access(r.w_off, r.w_len),
               n=r.n, direction=r.direction, ncols=r.ncols, nb1=r.nb1, half=r.half, real_input=r.real_input,
               out_keep=r.out_keep, same=r.same) for r in recs[:n]]


def ancestors(ops):
    """anc[i]: bit j set = operation j happens before operation i (the log order is a topological order of every edge)"""
    anc, last_on, host, last_record = [], {}, {}, {}
    signals = {}
    for i, o in enumerate(ops):
        preds = []
        if o.stream in last_on:
            preds.append(last_on[o.stream])                     # program order
        if o.rank in host:
            preds.append(host[o.rank])                          # behind the last host wait of this rank
        if o.kind == KIND["stream_wait"] and o.event in last_record:
            preds.append(last_record[o.event])
        if o.kind == KIND["flag_wait"]:
            hit = [j for j, v in signals.get(o.event, []) if v >= o.value]
            if hit:
                preds.append(hit[0])
        a = 0
        for p in preds:
            a |= anc[p] | (1 << p)
        anc.append(a)
        last_on[o.stream] = i
        if o.kind == KIND["event_record"]:
            last_record[o.event] = i
        elif o.kind == KIND["flag_signal"]:
            signals.setdefault(o.event, []).append((i, o.value))
        elif o.kind == KIND["stream_sync"]:
            host[o.rank] = i
    return anc


def _overlap(a, b):
    return a.size and b.size and np.intersect1d(a, b, assume_unique=True).size


def check(ops, allowed_syncs=()):
    """violations of the rules above, as strings (empty: the calls bracketed by marks are correctly ordered).  Every rank of the
    log needs one entry and one exit mark.  allowed_syncs: names of streams ("S", "side") on which a host wait is intended."""
    anc = ancestors(ops)
    out = []
    ranks = sorted({o.rank for o in ops})
    inside = []
    for r in ranks:
        marks = [(i, o) for i, o in enumerate(ops) if o.rank == r and o.kind == KIND["mark"]]
        ent = [i for i, o in marks if o.value == ENTRY]
        ext = [i for i, o in marks if o.value == EXIT]
        if len(ent) != 1 or len(ext) != 1:
            out.append(f"rank {r}: {len(ent)} entry and {len(ext)} exit marks in the log (one of each is needed)")
            continue
        e, x = ent[0], ext[0]
        S = ops[e].stream
        for i in range(e + 1, x):
            o = ops[i]
            if o.rank != r:
                continue
            if o.launch:
                inside.append(i)
                if not (anc[i] >> e) & 1:
                    out.append(f"fork: op {i} {o} is not ordered after the caller's stream at entry")
                if not (anc[x] >> i) & 1:
                    out.append(f"join: op {i} {o} is not ordered before the caller's stream at return")
            elif o.kind == KIND["stream_sync"]:
                which = "S" if o.stream == S else "side"
                if which not in allowed_syncs:
                    out.append(f"host wait: op {i} stream_sync on {'the caller stream' if which == 'S' else 'a side stream'} inside an async call")
    inside.sort()
    for ai, i in enumerate(inside):
        for j in inside[ai + 1:]:
            a, b = ops[i], ops[j]
            if a.stream == b.stream or (anc[j] >> i) & 1:
                continue
            for what, p, q in (("write/read", a.writes, b.reads), ("read/write", a.reads, b.writes), ("write/write", a.writes, b.writes)):
                if _overlap(p, q):
                    out.append(f"hazard: ops {i} {a} and {j} {b} are unordered and overlap ({what})")
                    break
    return out


def traced_transforms(CB, api, po, case, barrier, owner):
    """this rank's part of a case on a caller stream in async mode: the calls once as a warm-up (lazily made streams and the
    recorded inverse schedule exist afterwards), then again between an entry and an exit mark with access recording on.
    `owner` resets the log (ranks as threads share one) and gets the operations back; the caller frees the stream S behind the plan."""
    import oracle_lib as O
    L = api.lib()
    c = api.comm_dict(po)
    S = CB.cpu_backend_streams_new_stream()
    L.offt_hip_set_stream(po, S)
    L.offt_hip_set_async(po, 1)
    buf = np.zeros(api.local_elems(po), dtype=np.complex128)

    def fill():
        buf[:] = 0
        i0, i1, i2 = c["isize"]
        if i0 and i1 and i2:
            s0, s1, s2 = c["istride"]
            f = O.hash_field(i0, i1, i2, *c["istart"])
            if case.get("r2c"):   # real rows: scalar strides
                idx = np.arange(i0)[:, None, None] * 2 * s0 + np.arange(i1)[None, :, None] * 2 * s1 + np.arange(i2)[None, None, :]
                buf.view(np.float64)[idx.ravel()] = f.real.ravel()
            else:
                idx = np.arange(i0)[:, None, None] * s0 + np.arange(i1)[None, :, None] * s1 + np.arange(i2)[None, None, :] * s2
                buf[idx.ravel()] = f.ravel()
    ptr = buf.ctypes.data_as(C.c_void_p)
    calls = [-1, +1] if case.get("inv") else [-1] * int(case.get("repeat", 1))
    fill()
    for d in calls:
        api.offt_3d_execute_dir(po, ptr, ptr, d)
    fill()
    barrier()
    if owner:
        CB.cpu_backend_streams_reset()
        CB.cpu_backend_streams_record_access(1)
    barrier()
    CB.cpu_backend_streams_mark(S, ENTRY)
    for d in calls:
        api.offt_3d_execute_dir(po, ptr, ptr, d)
    CB.cpu_backend_streams_mark(S, EXIT)
    barrier()
    ops = read_log(CB) if owner else None
    if owner:
        CB.cpu_backend_streams_record_access(0)
    return ops, S


def gloo_main(cases, outdir):
    """one gloo rank per process: every rank checks its own log"""
    import torch.distributed as dist
    import cpu_world
    from offt_amd import api
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=size)
    cpu_world._cb_lib = streams_cb_lib
    out = []
    for case in cases:
        for k, v in case.get("env", {}).items():
            os.environ[k] = str(v)
        CB = cpu_world.install(rank, size, dist=dist)
        po = api.offt_3d_init(*case["N"], custom_params=api.make_params(**case["params"]), is_r2c=int(case.get("r2c", 0)))
        try:
            ops, S = traced_transforms(CB, api, po, case, dist.barrier, True)
        finally:
            api.offt_3d_fin(po)
        CB.cpu_backend_streams_free_stream(S)
        launches = [o for o in ops if o.launch]
        out.append({"case": case, "violations": check(ops), "ops": len(ops), "kinds": sorted({o.name for o in ops}),
                    "streams": len({o.stream for o in launches})})
        for k in case.get("env", {}):
            os.environ.pop(k, None)
        dist.barrier()
    cpu_world.uninstall()
    json.dump(out, open(os.path.join(outdir, f"gloo_rank{rank}.json"), "w"))
    dist.destroy_process_group()


# ---- ranks as threads on the CPU backend (the edge-drop controls) ---------------------------------------------------------
def world_main(size, cases, outpath):
    """every case: plan, caller stream, async; one warm-up forward (+ inverse), then the bracketed calls; all ranks' operations
    land in one log (direct stores reach into a peer's memory, flag edges cross ranks)"""
    import collections
    import threading
    import cpu_world
    from offt_amd import api
    cpu_world._cb_lib = streams_cb_lib
    L = cpu_world.test_lib()
    L.offt_hip_test_set_p2p.argtypes = [C.c_void_p, C.c_void_p]
    L.offt_hip_test_set_p2p.restype = None
    CB = streams_cb_lib()
    wire = {"cv": threading.Condition(), "q": collections.defaultdict(collections.deque), "failed": False}
    tls = threading.local()
    errors, results = [], []

    def fail():
        with wire["cv"]:
            wire["failed"] = True
            wire["cv"].notify_all()

    def transport(which, npeers, peer_in_group, sendp, sendbytes, recvp, recvbytes):
        try:
            rank, p1 = tls.rank, L.offt_hip_test_current_p1()
            acks = []
            for a in range(npeers):
                if sendbytes[a]:
                    ack = threading.Event()
                    with wire["cv"]:
                        wire["q"][(which, rank, cpu_world.group_peer(which, peer_in_group[a], rank, size, p1))].append((sendp[a], sendbytes[a], ack))
                        wire["cv"].notify_all()
                    acks.append(ack)
            for a in range(npeers):
                if recvbytes[a]:
                    key = (which, cpu_world.group_peer(which, peer_in_group[a], rank, size, p1), rank)
                    with wire["cv"]:
                        if not wire["cv"].wait_for(lambda: wire["q"][key] or wire["failed"], 60.0) or wire["failed"]:
                            raise RuntimeError(f"no message on {key}")
                        ptr, nb, ack = wire["q"][key].popleft()
                    assert nb == recvbytes[a]
                    C.memmove(recvp[a], ptr, nb)
                    ack.set()
            for ack in acks:
                if not ack.wait(60.0):
                    raise RuntimeError("send not consumed")
            return 0
        except Exception as e:
            print("transport failed:", repr(e), flush=True)
            fail()
            return -1

    book = {"cv": threading.Condition(), "posted": {}, "count": collections.defaultdict(int)}

    def peer_open(which, npeers, self_idx, local, nbytes, peers):
        try:
            rank, p1 = tls.rank, L.offt_hip_test_current_p1()
            members = [cpu_world.group_peer(which, g, rank, size, p1) for g in range(npeers)]
            gid = (which, members[0])
            with book["cv"]:
                seq = book["count"][(gid, rank)]
                book["count"][(gid, rank)] += 1
                book["posted"][(gid, seq, rank)] = local
                book["cv"].notify_all()
                if not book["cv"].wait_for(lambda: all((gid, seq, m) in book["posted"] for m in members) or wire["failed"], 60.0) or wire["failed"]:
                    return -1
                for g, m in enumerate(members):
                    peers[g] = book["posted"][(gid, seq, m)]
            return 0
        except Exception as e:
            print("peer_open failed:", repr(e), flush=True)
            fail()
            return -1

    hook_bar = {}

    def hook():
        try:
            hook_bar["b"].wait(60.0)
        except threading.BrokenBarrierError:
            fail()

    PEER_CB = C.CFUNCTYPE(C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p))
    a2a_cb, peer_cb, hook_cb = cpu_world.A2A_CB(transport), PEER_CB(peer_open), C.CFUNCTYPE(None)(hook)
    CB.cpu_backend_set_a2a(a2a_cb)
    CB.cpu_backend_set_peer_open(C.cast(peer_cb, C.c_void_p))

    def rank_thread(rank, case, bar):
        try:
            tls.rank = rank
            CB.cpu_backend_streams_set_rank(rank)
            L.offt_hip_test_set_backend(CB.cpu_backend_table(), rank, size)
            if case.get("p2p"):
                L.offt_hip_test_set_p2p(C.cast(peer_cb, C.c_void_p), C.cast(hook_cb, C.c_void_p))
            po = api.offt_3d_init(*case["N"], custom_params=api.make_params(**case["params"]), is_r2c=int(case.get("r2c", 0)))
            ops, S = traced_transforms(CB, api, po, case, bar.wait, rank == 0)
            if rank == 0:
                results.append({"case": case, "violations": check(ops), "ops": len(ops), "kinds": sorted({o.name for o in ops})})
            bar.wait()
            api.offt_3d_fin(po)
            CB.cpu_backend_streams_free_stream(S)
            L.offt_hip_test_set_p2p(None, None)
            L.offt_hip_test_set_backend(None, 0, 1)
        except Exception as e:
            errors.append((rank, repr(e)))
            fail()
            for b in (bar, hook_bar.get("b")):
                try:
                    b.abort()
                except Exception:
                    pass

    for case in cases:
        for k, v in case.get("env", {}).items():
            os.environ[k] = str(v)
        if case.get("p2p"):
            os.environ["OFFT_EXCHANGE"] = "p2p"
        bar = threading.Barrier(size)
        hook_bar["b"] = threading.Barrier(size)
        book["posted"].clear()
        book["count"].clear()
        th = [threading.Thread(target=rank_thread, args=(r, case, bar)) for r in range(size)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for k in case.get("env", {}):
            os.environ.pop(k, None)
        os.environ.pop("OFFT_EXCHANGE", None)
        if errors:
            print("FAILED", errors, flush=True)
            sys.exit(1)
    json.dump(results, open(outpath, "w"))


if __name__ == "__main__":
    if sys.argv[1] == "world":
        world_main(int(sys.argv[2]), json.loads(sys.argv[3]), sys.argv[4])
    elif sys.argv[1] == "gloo":
        gloo_main(json.loads(sys.argv[2]), sys.argv[3])
