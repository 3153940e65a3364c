# Build the MI355X OFFT library (HIP kernels + C host) and the test oracle.
#   make            -> offt_amd/liboffthip.so, oracle/liboracle.so
#   make harness    -> bin/run-fft (C harness, links the HIP runtime explicitly)
ROCM      ?= /opt/rocm
HIPCC     ?= $(ROCM)/bin/hipcc
CC        ?= gcc
ARCH      ?= gfx950
CSRC      := offt_amd/csrc
BUILD     := build
HIPFLAGS  := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -I$(CSRC) -Iinclude -I$(BUILD)
CFLAGS    := -std=gnu11 -O2 -g -Wall -Wextra -fPIC -I$(ROCM)/include -I$(CSRC) -Iinclude

all: offt_amd/liboffthip.so oracle/liboracle.so tests/liboffthip_test.so tools/liboffthip_diag.so

$(BUILD):
	mkdir -p $(BUILD)

# the kernel instantiations are grouped into several translation units so that `make -j` compiles them in parallel
HIPSRC    := offt_reg_pow2_f32_big offt_kernels offt_reg_pow2_f64 offt_reg_pow2_f64_1024 offt_reg_pair_yx_f64 offt_reg_pow2_f64_anysplit offt_reg_pow2_f32 offt_reg_pow2_f32_anysplit offt_reg_pow2_f32_pair offt_reg_pow2_tw4 offt_reg_mixed_f64_a offt_reg_mixed_f64_b \
             offt_reg_mixed_f64_c offt_reg_mixed_f64_d offt_reg_mixed_f64_e offt_reg_mixed_f32_a offt_reg_mixed_f32_b offt_reg_bluestein offt_reg_bluestein_f32 \
             offt_reg_conv_f64 offt_reg_conv_f32 offt_reg_conv_oop_f64 offt_reg_conv_oop_f32 offt_reg_conv_mixed_f64 offt_reg_conv_mixed_f32 offt_reg_conv_oop_mixed_f64 offt_reg_conv_oop_mixed_f32 offt_reg_conv_sum_f64 offt_reg_conv_sum_f32 offt_reg_conv_sum_mixed_f64 offt_reg_conv_sum_mixed_f32 offt_reg_spec_f64 offt_reg_spec_f32 offt_reg_spec_mixed_f64 offt_reg_spec_mixed_f32 offt_reg_half_f64 offt_reg_half_f32 offt_reg_half_real_f64 offt_reg_half_real_f32 \
             offt_reg_half_mixed_f64 offt_reg_half_mixed_f32 offt_reg_half_real_mixed_f64 offt_reg_half_real_mixed_f32 offt_reg_prod_f64 offt_reg_prod_f32 \
             offt_reg_prod_real_f64 offt_reg_prod_real_f32
HIPOBJ    := $(HIPSRC:%=$(BUILD)/%.o)
$(BUILD)/%.o: $(CSRC)/%.hip $(CSRC)/offt_panel.hpp $(CSRC)/offt_bluestein.hpp $(CSRC)/offt_hipk.h $(CSRC)/offt_w32_consts.h $(CSRC)/offt_wr_consts.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $(BUILD)/$*.resource_usage.txt || (cat $(BUILD)/$*.resource_usage.txt; false)

# the device part of offt_panel.hpp as a string inside the library: plan-time specialisation through hipRTC
$(BUILD)/offt_rtc_source.inc: $(CSRC)/offt_panel.hpp $(CSRC)/offt_hipk.h $(CSRC)/offt_w32_consts.h $(CSRC)/offt_wr_consts.h tools/gen_rtc_source.py | $(BUILD)
	python3 tools/gen_rtc_source.py $@
$(BUILD)/offt_kernels.o: $(BUILD)/offt_rtc_source.inc

$(BUILD)/offt_host.o: $(CSRC)/offt_host.c $(CSRC)/offt_hipk.h $(CSRC)/offt_backend.h include/offt.h include/offt_hip.h | $(BUILD)
	$(CC) $(CFLAGS) -c $< -o $@

# The HIP runtime is deliberately NOT a DT_NEEDED entry: the hosting process
# decides which libamdhip64 is in use (PyTorch bundles its own); C programs link
# -lamdhip64 themselves.
offt_amd/liboffthip.so: $(HIPOBJ) $(BUILD)/offt_host.o
	g++ -shared -o $@ $^ -Wl,--allow-shlib-undefined -Wl,-Bsymbolic -ldl -lm -lpthread

# TEST build of the same library: identical kernel objects, the host compiled with -DOFFT_TEST_SEAMS, which adds the two
# test-only entry points of offt_backend.h (CPU descriptor interpreter for the host-logic tests, host-staged transport
# for several ranks on one GPU).  The product library above does not contain them.
$(BUILD)/offt_host_test.o: $(CSRC)/offt_host.c $(CSRC)/offt_hipk.h $(CSRC)/offt_backend.h include/offt.h include/offt_hip.h | $(BUILD)
	$(CC) $(CFLAGS) -DOFFT_TEST_SEAMS -c $< -o $@
tests/liboffthip_test.so: $(HIPOBJ) $(BUILD)/offt_host_test.o
	g++ -shared -o $@ $^ -Wl,--allow-shlib-undefined -Wl,-Bsymbolic -ldl -lm -lpthread

# DIAGNOSTICS build for launchers (bench.py's exchange-only / compute-only split of a multi-rank run): the product plus
# offt_hip_set_debug_skip, which makes an execute leave out its passes or its exchanges.  Never the measured library.
$(BUILD)/offt_host_diag.o: $(CSRC)/offt_host.c $(CSRC)/offt_hipk.h $(CSRC)/offt_backend.h include/offt.h include/offt_hip.h | $(BUILD)
	$(CC) $(CFLAGS) -DOFFT_BENCH_DIAGNOSTICS -c $< -o $@
tools/liboffthip_diag.so: $(HIPOBJ) $(BUILD)/offt_host_diag.o
	g++ -shared -o $@ $^ -Wl,--allow-shlib-undefined -Wl,-Bsymbolic -ldl -lm -lpthread

oracle/liboracle.so: oracle/oracle_fft.c oracle/oracle_offt.c oracle/oracle.h
	$(CC) -std=gnu11 -O3 -fopenmp -fPIC -shared -Ioracle -o $@ oracle/oracle_fft.c oracle/oracle_offt.c -lm

clean:
	rm -rf $(BUILD) offt_amd/liboffthip.so tests/liboffthip_test.so tools/liboffthip_diag.so oracle/liboracle.so bin

.PHONY: all clean

# test-only CPU interpreter of pass descriptors (never linked into the product)
tests/libcpubackend.so: tests/cpu_backend.c oracle/oracle_fft.c oracle/oracle.h offt_amd/csrc/offt_backend.h
	$(CC) -std=gnu11 -O2 -fPIC -shared -Ioracle -Ioffamd -I$(CSRC) -o $@ tests/cpu_backend.c oracle/oracle_fft.c -lm

# ... and the same interpreter with the two convolution entries of the table filled (tests/test_convolve.py)
tests/libcpubackend_conv.so: tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c oracle/oracle.h offt_amd/csrc/offt_backend.h offt_amd/csrc/offt_hipk.h
	$(CC) -std=gnu11 -O2 -fPIC -shared -Ioracle -I$(CSRC) -o $@ tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c -lm

# ... and with offt_pass_desc::half interpreted and the zero_outside entry filled (tests/test_half_box.py)
tests/libcpubackend_pad.so: tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c oracle/oracle.h offt_amd/csrc/offt_backend.h offt_amd/csrc/offt_hipk.h
	$(CC) -std=gnu11 -O2 -fPIC -shared -Ioracle -I$(CSRC) -o $@ tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c -lm

# ... and with the two real ends of a half-box chain interpreted (real_input together with half; tests/test_half_box_r2c.py)
tests/libcpubackend_padreal.so: tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c oracle/oracle.h offt_amd/csrc/offt_backend.h offt_amd/csrc/offt_hipk.h
	$(CC) -std=gnu11 -O2 -fPIC -shared -Ioracle -I$(CSRC) -o $@ tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c -lm

# ... and with bit 4 of half (the permission for the mixed-radix real-row kernels) understood (tests/test_half_box_r2c_mixed.py)
tests/libcpubackend_padreal_mixed.so: tests/cpu_backend_padreal_mixed.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c oracle/oracle.h offt_amd/csrc/offt_backend.h offt_amd/csrc/offt_hipk.h
	$(CC) -std=gnu11 -O2 -fPIC -shared -Ioracle -I$(CSRC) -o $@ tests/cpu_backend_padreal_mixed.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c -lm

# ... and with the two entries of the multi-output convolution filled and every launch logged (tests/test_convolve_multi.py)
tests/libcpubackend_multi.so: tests/cpu_backend_multi.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c oracle/oracle.h offt_amd/csrc/offt_backend.h offt_amd/csrc/offt_hipk.h
	$(CC) -std=gnu11 -O2 -fPIC -shared -Ioracle -I$(CSRC) -o $@ tests/cpu_backend_multi.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c -lm

# ... and with the two entries of the multi-input convolution filled and every launch logged (tests/test_convolve_sum.py)
tests/libcpubackend_sum.so: tests/cpu_backend_sum.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c oracle/oracle.h offt_amd/csrc/offt_backend.h offt_amd/csrc/offt_hipk.h
	$(CC) -std=gnu11 -O2 -fPIC -shared -Ioracle -I$(CSRC) -o $@ tests/cpu_backend_sum.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c -lm

# ... and with the two entries of the filtered transforms filled and every launch logged (tests/test_spectral_filtered.py)
tests/libcpubackend_spec.so: tests/cpu_backend_spec.c tests/cpu_backend_multi.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c oracle/oracle.h offt_amd/csrc/offt_backend.h offt_amd/csrc/offt_hipk.h
	$(CC) -std=gnu11 -O2 -fPIC -shared -Ioracle -I$(CSRC) -o $@ tests/cpu_backend_spec.c tests/cpu_backend_multi.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c -lm

# ... and with the entry of the shell-binned spectra filled and its calls counted (tests/test_spectrum_shells.py)
tests/libcpubackend_shells.so: tests/cpu_backend_shells.c tests/cpu_backend_spec.c tests/cpu_backend_multi.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c oracle/oracle.h offt_amd/csrc/offt_backend.h offt_amd/csrc/offt_hipk.h
	$(CC) -std=gnu11 -O2 -fPIC -shared -Ioracle -I$(CSRC) -o $@ tests/cpu_backend_shells.c tests/cpu_backend_spec.c tests/cpu_backend_multi.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c -lm

# ... and with the two entries of the pseudo-spectral product filled and every launch logged (tests/test_product.py)
tests/libcpubackend_prod.so: tests/cpu_backend_prod.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c oracle/oracle.h offt_amd/csrc/offt_backend.h offt_amd/csrc/offt_hipk.h
	$(CC) -std=gnu11 -O2 -fPIC -shared -Ioracle -I$(CSRC) -o $@ tests/cpu_backend_prod.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c -lm

# ... and with the real-row fused launch of the product (prod_pass_real) interpreted from its definition and logged (tests/test_product_real.py)
tests/libcpubackend_prod_real.so: tests/cpu_backend_prod_real.c tests/cpu_backend_prod.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c oracle/oracle.h offt_amd/csrc/offt_backend.h offt_amd/csrc/offt_hipk.h
	$(CC) -std=gnu11 -O2 -fPIC -shared -Ioracle -I$(CSRC) -o $@ tests/cpu_backend_prod_real.c tests/cpu_backend_prod.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c -lm

# ... and with every launch, event and stream operation logged with its stream, and the memory each launch touches (tests/test_streams.py)
tests/libcpubackend_streams.so: tests/cpu_backend_streams.c tests/cpu_backend_spec.c tests/cpu_backend_sum.c tests/cpu_backend_multi.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c oracle/oracle.h offt_amd/csrc/offt_backend.h offt_amd/csrc/offt_hipk.h
	$(CC) -std=gnu11 -O2 -fPIC -shared -Ioracle -I$(CSRC) -o $@ tests/cpu_backend_streams.c tests/cpu_backend_spec.c tests/cpu_backend_sum.c tests/cpu_backend_multi.c tests/cpu_backend_padreal.c tests/cpu_backend_pad.c tests/cpu_backend_conv.c tests/cpu_backend.c oracle/oracle_fft.c -lm -lpthread

# ... and the plain interpreter with offt_backend::pass_pair and a log of the passes (tests/test_zgroup_pipeline.py)
tests/libcpubackend_pipeline.so: tests/cpu_backend_pipeline.c tests/cpu_backend.c oracle/oracle_fft.c oracle/oracle.h offt_amd/csrc/offt_backend.h offt_amd/csrc/offt_hipk.h
	$(CC) -std=gnu11 -O2 -fPIC -shared -Ioracle -I$(CSRC) -o $@ tests/cpu_backend_pipeline.c tests/cpu_backend.c oracle/oracle_fft.c -lm

# ... and the plain interpreter with pass_pair, every launch and stream operation logged with its stream, and a replay that
# runs the queued operations in the orders the event edges allow (tests/test_zgroup_chains.py)
tests/libcpubackend_chains.so: tests/cpu_backend_chains.c tests/cpu_backend.c oracle/oracle_fft.c oracle/oracle.h offt_amd/csrc/offt_backend.h offt_amd/csrc/offt_hipk.h
	$(CC) -std=gnu11 -O2 -fPIC -shared -Ioracle -I$(CSRC) -o $@ tests/cpu_backend_chains.c tests/cpu_backend.c oracle/oracle_fft.c -lm

# run-fft-compatible C harness.  MPI=1 builds the multi-rank variant
# against an MPI found at MPI_PREFIX (e.g. /opt/conda; linked by file name, not -L: a conda lib directory also holds an
# older libstdc++ that must not shadow the system one the HIP runtime needs).
MPI_PREFIX ?= /opt/conda
harness: bin/run-fft
bin/run-fft: harness/run-fft.c offt_amd/liboffthip.so
	mkdir -p bin
ifeq ($(MPI),1)
	$(CC) -std=gnu11 -O2 -Wall -DOFFT_HARNESS_MPI -Iinclude -I$(MPI_PREFIX)/include -o $@ harness/run-fft.c -Lofft_amd -loffthip -L$(ROCM)/lib -lamdhip64 $(MPI_PREFIX)/lib/libmpi.so -lm -Wl,-rpath-link,/usr/lib/x86_64-linux-gnu -Wl,-rpath,'$$ORIGIN/../offt_amd' -Wl,-rpath,$(ROCM)/lib -Wl,-rpath,$(MPI_PREFIX)/lib
else
	$(CC) -std=gnu11 -O2 -Wall -Iinclude -o $@ harness/run-fft.c -Lofft_amd -loffthip -L$(ROCM)/lib -lamdhip64 -lm -Wl,-rpath,'$$ORIGIN/../offt_amd' -Wl,-rpath,$(ROCM)/lib
endif

# the registry queries of offt_hipk.h under AddressSanitizer + UBSan in a stand-alone program (tools/registry_dump.cpp): the
# HOST side of every kernel source is compiled again with the sanitizers around the device code of the product object; the
# program launches nothing and needs no GPU.  Its output is kept for comparing two builds.
ASANREG   := $(BUILD)/asan_registry
$(ASANREG)/%.o: $(CSRC)/%.hip $(BUILD)/%.o
	mkdir -p $(ASANREG)
	$(ROCM)/lib/llvm/bin/llvm-objcopy --dump-section .hip_fatbin=$(ASANREG)/$*.fatbin $(BUILD)/$*.o
	$(HIPCC) --offload-arch=$(ARCH) --cuda-host-only -Xclang -fcuda-include-gpubinary -Xclang $(ASANREG)/$*.fatbin -O1 -g -std=c++17 \
	  -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -I$(CSRC) -Iinclude -I$(BUILD) -c $< -o $@
asan-registry: $(HIPSRC:%=$(ASANREG)/%.o) tools/registry_dump.cpp
	$(ROCM)/lib/llvm/bin/clang++ -O1 -g -fsanitize=address,undefined -I$(CSRC) tools/registry_dump.cpp $(HIPSRC:%=$(ASANREG)/%.o) -o $(ASANREG)/registry_dump \
	  -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,$(ROCM)/lib -ldl -lpthread
	$(ASANREG)/registry_dump > $(ASANREG)/registry_dump.txt
	@echo "asan-registry: clean, `wc -l < $(ASANREG)/registry_dump.txt` answers in $(ASANREG)/registry_dump.txt"

# host logic under AddressSanitizer + UBSan on the CPU test backend (GPU ASan is not available on the pool)
asan-test: $(HIPOBJ)
	mkdir -p $(BUILD)/asan
	$(CC) -std=gnu11 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -fPIC -DOFFT_TEST_SEAMS -I$(ROCM)/include -I$(CSRC) -Iinclude -c $(CSRC)/offt_host.c -o $(BUILD)/asan/offt_host.o
	g++ -shared -fsanitize=address,undefined -o $(BUILD)/asan/liboffthip.so $(HIPOBJ) $(BUILD)/asan/offt_host.o -Wl,--allow-shlib-undefined -ldl -lm -lpthread
	$(CC) -std=gnu11 -O1 -g -fsanitize=address,undefined -fPIC -shared -Ioracle -I$(CSRC) -o $(BUILD)/asan/libcpubackend.so tests/cpu_backend.c oracle/oracle_fft.c -lm
	cp tests/libcpubackend.so $(BUILD)/asan/libcpubackend.so.orig
	cp $(BUILD)/asan/libcpubackend.so tests/libcpubackend.so
	LD_PRELOAD="$$($(CC) -print-file-name=libasan.so) $$($(CC) -print-file-name=libubsan.so)" ASAN_OPTIONS=detect_leaks=0 \
	  OFFT_AMD_TEST_LIB=$(CURDIR)/$(BUILD)/asan/liboffthip.so python -m pytest tests/test_host_logic.py tests/test_p2p_world.py -x -q; \
	  rc=$$?; cp $(BUILD)/asan/libcpubackend.so.orig tests/libcpubackend.so; exit $$rc
