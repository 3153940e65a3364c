"""Several ranks sharing the one GPU, real-input plans: forward r2c, then the complex-to-real inverse with output scale 1/N
must give back every rank's input block (launched by test_c2r.py).

  _c2r_world.py <size> <cases.json> <outdir>        ranks as THREADS of one process, the test build's transport seam
                                                     (the staged exchange copies device to device; "p2p": 1 the
                                                     direct-store exchange through the peer-open seam)
  _c2r_world.py proc <case.json> <outdir>           one rank per PROCESS (RANK / WORLD_SIZE / MASTER_* set), the exchange
                                                     host-staged over gloo, or with "p2p": 1 the product's hipIpc path

A case: {"N": [Nx, Ny, Nz], "params": {...}, "f32": 0/1, "p2p": 0/1, "k1": K1 streams, "comm": comm streams}.  The summary
(threads) or per-rank record (processes) holds the worst rank's rel-L2 distance from its input block."""
import ctypes as C
import json
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

OPT_COMM_STREAMS, OPT_K1_STREAMS = 3, 5  # include/offt_hip.h


def roundtrip(L, api, torch, po, case):
    """fill (seeded hash) -> forward -> c2r with scale 1/N: rel-L2 of the real rows against the input block"""
    c = api.comm_dict(po)
    f32 = bool(case.get("f32"))
    td = torch.float32 if f32 else torch.float64
    if case.get("k1"):
        L.offt_hip_set_option(po, OPT_K1_STREAMS, int(case["k1"]))
    if case.get("comm"):
        L.offt_hip_set_option(po, OPT_COMM_STREAMS, int(case["comm"]))
    n = 2 * api.local_elems(po)
    a = torch.zeros(n, dtype=td, device="cuda")
    torch.cuda.synchronize()
    if L.offt_hip_fill_input(po, a.data_ptr(), 1):
        raise RuntimeError("fill failed")
    torch.cuda.synchronize()
    want = a.cpu().numpy().astype(np.float64)
    api.offt_3d_execute(po, a.data_ptr(), a.data_ptr())
    L.offt_hip_set_output_scale(po, 1.0 / float(np.prod(case["N"])))
    api.offt_3d_execute_dir(po, a.data_ptr(), a.data_ptr(), +1)
    torch.cuda.synchronize()
    got = a.cpu().numpy().astype(np.float64)
    n0, n1, n2 = c["isize"]
    s0, s1, _ = c["istride"]
    idx = (np.arange(n0)[:, None, None] * 2 * s0 + np.arange(n1)[None, :, None] * 2 * s1 + np.arange(n2)[None, None, :]).ravel()
    if idx.size == 0:
        return 0.0, c
    return float(np.linalg.norm(got[idx] - want[idx]) / np.linalg.norm(want[idx])), c


def bind(L):
    L.offt_hip_set_option.argtypes = [C.c_void_p, C.c_int, C.c_longlong]
    L.offt_hip_set_output_scale.argtypes = [C.c_void_p, C.c_double]
    L.offt_hip_set_output_scale.restype = None
    L.offt_hip_get_exchange.argtypes = [C.c_void_p]


def threads_main(size, cases, outdir):
    import torch
    import cpu_world
    from _thread_world import Wire, PEER_CB, HOOK_CB
    from offt_amd import api
    torch.cuda.set_device(0)
    L = cpu_world.test_lib()
    bind(L)
    L.offt_hip_test_set_p2p.argtypes = [C.c_void_p, C.c_void_p]
    L.offt_hip_test_set_p2p.restype = None
    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    tls = threading.local()
    summary = []
    for ci, case in enumerate(cases):
        wire = Wire()
        results, errors = {}, []
        book = {"cv": threading.Condition(), "posted": {}, "count": {}}
        hook_bar = threading.Barrier(size)

        def peer_open(which, npeers, self_idx, local, nbytes, peers):
            try:
                rank = tls.rank
                members = [cpu_world.group_peer(which, g, rank, size, L.offt_hip_test_current_p1()) for g in range(npeers)]
                gid = (which, members[0])
                with book["cv"]:
                    seq = book["count"].get((gid, rank), 0)
                    book["count"][(gid, rank)] = seq + 1
                    book["posted"][(gid, seq, rank)] = (local, nbytes)
                    book["cv"].notify_all()
                    if not book["cv"].wait_for(lambda: all((gid, seq, m) in book["posted"] for m in members) or wire.failed, 120.0) or wire.failed:
                        return -1
                    for g, m in enumerate(members):
                        peers[g] = book["posted"][(gid, seq, m)][0]
                return 0
            except Exception as e:
                print("peer_open failed:", repr(e), flush=True)
                wire.fail()
                return -1

        def hook():
            try:
                hook_bar.wait(120.0)
            except threading.BrokenBarrierError:
                wire.fail()

        peer_cb, hook_cb = PEER_CB(peer_open), HOOK_CB(hook)

        def make_transport(rank):
            def transport(which, npeers, peer_in_group, sendp, sendbytes, recvp, recvbytes):
                try:
                    p1 = L.offt_hip_test_current_p1()
                    acks = []
                    for a in range(npeers):
                        if sendbytes[a]:
                            peer = cpu_world.group_peer(which, peer_in_group[a], rank, size, p1)
                            acks.append(wire.post((which, rank, peer), sendp[a], sendbytes[a]))
                    for a in range(npeers):
                        if recvbytes[a]:
                            peer = cpu_world.group_peer(which, peer_in_group[a], rank, size, p1)
                            ptr, nb, ack = wire.take((which, peer, rank))
                            assert nb == recvbytes[a]
                            if hip.hipMemcpy(recvp[a], ptr, nb, 3) != 0:
                                raise RuntimeError("hipMemcpy failed")
                            L.offt_hip_device_synchronize()
                            ack.set()
                    for ack in acks:
                        if not ack.wait(120.0):
                            raise RuntimeError("send not consumed")
                    return 0
                except Exception as e:
                    print("transport failed on rank", rank, repr(e), flush=True)
                    wire.fail()
                    return -1
            return transport

        cbs = {r: cpu_world.A2A_CB(make_transport(r)) for r in range(size)}
        bar = threading.Barrier(size)
        if case.get("p2p"):
            os.environ["OFFT_EXCHANGE"] = "p2p"

        def rank_thread(rank):
            try:
                tls.rank = rank
                L.offt_hip_test_set_transport(C.cast(cbs[rank], C.c_void_p), rank, size)
                if case.get("p2p"):
                    L.offt_hip_test_set_p2p(C.cast(peer_cb, C.c_void_p), C.cast(hook_cb, C.c_void_p))
                prec = api.F32 if case.get("f32") else api.F64
                po = api.offt_3d_init(*case["N"], custom_params=api.make_params(**case["params"]), is_equalxy=case.get("eq", 0),
                                      is_r2c=1, precision=prec)
                if case.get("p2p") and L.offt_hip_get_exchange(po) != 1:
                    raise RuntimeError("the plan fell back to the staged exchange")
                bar.wait(120.0)
                results[rank] = roundtrip(L, api, torch, po, case)[0]
                bar.wait(120.0)
                api.offt_3d_fin(po)
                L.offt_hip_test_set_p2p(None, None)
                L.offt_hip_test_set_transport(None, 0, 1)
            except Exception as e:
                errors.append((rank, repr(e)))
                wire.fail()
                for b in (bar, hook_bar):
                    try:
                        b.abort()
                    except Exception:
                        pass

        th = [threading.Thread(target=rank_thread, args=(r,)) for r in range(size)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        os.environ.pop("OFFT_EXCHANGE", None)
        torch.cuda.synchronize()
        if errors:
            print("FAILED", case, errors, flush=True)
            sys.exit(1)
        rec = {"case": case, "size": size, "rel": max(results.values()), "tol": 5e-6 if case.get("f32") else 1e-13}
        print(json.dumps(rec), flush=True)
        summary.append(rec)
    json.dump(summary, open(os.path.join(outdir, "summary.json"), "w"))


def proc_main(case, outdir):
    import torch
    import torch.distributed as dist
    import cpu_world
    from offt_amd import api
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=size)
    torch.cuda.set_device(0)
    L = cpu_world.test_lib()
    bind(L)

    def transport(which, npeers, peer_in_group, sendp, sendbytes, recvp, recvbytes):
        try:
            reqs, pend = [], []
            for a in range(npeers):
                peer = cpu_world.group_peer(which, peer_in_group[a], rank, size, L.offt_hip_test_current_p1())
                sb, rb = sendbytes[a], recvbytes[a]
                if peer == rank:
                    if sb:
                        tmp = (C.c_char * sb)()
                        L.offt_hip_memcpy_d2h(tmp, sendp[a], sb)
                        L.offt_hip_memcpy_h2d(recvp[a], tmp, sb)
                    continue
                if rb:
                    t = torch.empty(rb, dtype=torch.uint8)
                    pend.append((t, recvp[a], rb))
                    reqs.append(dist.irecv(t, src=peer, tag=which))
                if sb:
                    t = torch.empty(sb, dtype=torch.uint8)
                    L.offt_hip_memcpy_d2h(C.c_void_p(t.data_ptr()), sendp[a], sb)
                    pend.append((t, None, 0))
                    reqs.append(dist.isend(t, dst=peer, tag=which))
            for r in reqs:
                r.wait()
            for t, dst, nb in pend:
                if dst is not None:
                    L.offt_hip_memcpy_h2d(dst, C.c_void_p(t.data_ptr()), nb)
            return 0
        except Exception as e:
            print("transport failed:", repr(e), flush=True)
            return -1

    cb = cpu_world.A2A_CB(transport)
    L.offt_hip_test_set_transport(C.cast(cb, C.c_void_p), rank, size)
    if case.get("p2p"):
        os.environ["OFFT_EXCHANGE"] = "p2p"
    po = api.offt_3d_init(*case["N"], custom_params=api.make_params(**case["params"]), is_equalxy=case.get("eq", 0), is_r2c=1,
                          precision=api.F32 if case.get("f32") else api.F64)
    os.environ.pop("OFFT_EXCHANGE", None)
    exchange = L.offt_hip_get_exchange(po)
    err, c = roundtrip(L, api, torch, po, case)
    api.offt_3d_fin(po)
    json.dump({"rel": err, "exchange": exchange, "comm": c}, open(os.path.join(outdir, f"proc_rank{rank}.json"), "w"))
    dist.barrier()
    L.offt_hip_test_set_transport(None, 0, 1)
    dist.destroy_process_group()


if __name__ == "__main__":
    if sys.argv[1] == "proc":
        proc_main(json.loads(sys.argv[2]), sys.argv[3])
    else:
        threads_main(int(sys.argv[1]), json.loads(sys.argv[2]), sys.argv[3])
