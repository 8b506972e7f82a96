# `make san` (fthmc_amd/csrc/Makefile): the recipe of the host-side sanitizer build.  Listed in .gpurunignore: the GPU pool refuses
# snapshots whose build files ask for sanitizers.
include Makefile

# Sanitizer build of the HOST side (never run on a GPU box): the host pass of every source with AddressSanitizer + UBSan
# (-Xarch_host: the device pass is what the product builds), launches / copies / memsets as succeeding no-ops (-DFT_DRYRUN,
# common.h), and the operator library against it.  tests/test_sanitizer.py loads them under the ASan runtime and takes every
# entry point through its argument checks, workspace carving and launch sequencing.
SANDIR = /tmp/fthmc_san
SANOUT = ../libfthmc_hip_san.so
SANTORCH = ../libfthmc_torch_san.so
SANFLAGS = -O1 -g -fno-omit-frame-pointer -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -DFT_DRYRUN -Wno-unused
# the operator library is built by clang++ here (ONE sanitizer runtime in the process): -fclang-abi-compat=17 keeps the mangling of
# PyTorch's enable_if templates the one g++ gave libtorch; -asan-globals=0: libstdc++'s header string constants exist in the
# uninstrumented libtorch too, instrumented twins of them trip the runtime's global registration
SANRT := $(shell ls $(ROCM)/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so 2>/dev/null | head -1)
san_build:
	mkdir -p $(SANDIR)
	for f in $(SRCS:.hip=); do $(HIPCC) -std=c++17 -fPIC --offload-arch=$(ARCH) $(SANFLAGS) -DFTHMC_SRC_SHA=\"$(SRC_SHA)\" -c $$f.hip -o $(SANDIR)/$$f.o & done; wait
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -Xarch_host -fsanitize=address,undefined -shared-libsan -o $(SANOUT) $(SRCS:%.hip=$(SANDIR)/%.o)
ifneq ($(TORCHDIR),)
	$(ROCM)/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fPIC -shared -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan -fclang-abi-compat=17 -mllvm -asan-globals=0 \
	  -D_GLIBCXX_USE_CXX11_ABI=$(TORCHABI) -D__HIP_PLATFORM_AMD__=1 -DUSE_ROCM=1 \
	  -I$(TORCHDIR)/include -I$(TORCHDIR)/include/torch/csrc/api/include -I$(ROCM)/include torch_library.cpp -o $(SANTORCH) \
	  -L.. -lfthmc_hip_san -L$(TORCHDIR)/lib -ltorch -ltorch_cpu -lc10 -lc10_hip -ltorch_hip -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,$(TORCHDIR)/lib
endif
	@echo "sanitizer runtime to preload: $(SANRT)"

# The schedule header on its own (integrator.h: plain C++): tests/hip/integrator_walk.cpp as a stand-alone program with the
# sanitizer runtimes linked in (nothing to preload), built where SANWALK says and run by tests/test_integrators.py
SANWALK ?= $(SANDIR)/integrator_walk
san_integrator:
	mkdir -p $(dir $(SANWALK))
	$(ROCM)/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	  -I. ../../tests/hip/integrator_walk.cpp -o $(SANWALK)

# The stand-alone walkers of the entry points, tests/hip/<name>_walk.cpp: `make -f san.mk san_<name>` builds one where SANEXE says
# (or the variable the walker's test has always passed: SANWALKVARS; default $(SANDIR)/<name>_walk), against the host-side sanitizer build of the library (built first when it is missing or older than a source), the sanitizer
# runtimes linked in (nothing to preload).  tempering (fthmc_ft_trajectory_pb_v, fthmc_hmc_trajectory_pb, fthmc_replica_swap,
# fthmc_ladder_init: tests/test_tempering.py), loops (the Wilson-loop entry points: tests/test_wilson_loops.py), local
# (fthmc_local_update: tests/test_local_update.py), instanton (the instanton hits and the integer reductions of topo_int.h:
# tests/test_instanton.py), meta (the fthmc_meta_* entry points: tests/test_meta.py), ft_meta (the fthmc_ft_meta_* entry points:
# tests/test_ft_meta.py), ft_defect (the fthmc_ft_defect_* entry points: tests/test_ft_defect.py, through SANEXE).  san_build, san_integrator and san_layout are rules of their own.
$(SANOUT): $(SRCS) common.h kernels.h integrator.h topo_int.h meta_tab.h api_call.h ../../include/fthmc_hip.h san.mk
	@$(MAKE) --no-print-directory -f san.mk san_build
SANWALKVARS = tempering:SANTEMP loops:SANLOOPS local:SANLOCAL instanton:SANINST meta:SANMETA ft_meta:SANFTMETA
SANEXE ?= $(or $($(patsubst $*:%,%,$(filter $*:%,$(SANWALKVARS)))),$(SANDIR)/$*_walk)
san_%: $(SANOUT)
	mkdir -p $(dir $(SANEXE))
	$(ROCM)/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan \
	  ../../tests/hip/$*_walk.cpp -o $(SANEXE) -L.. -lfthmc_hip_san -Wl,-rpath,$(abspath ..) -Wl,-rpath,$(dir $(SANRT))

# The workspace layouts of api_call.h (ws_layout, vjp_layout, force_layout on one carver): tests/hip/layout_walk.cpp includes the
# header itself (hipcc's host pass: the header pulls in the HIP headers) with the unsigned-overflow check on top, and asks the
# library's size queries in the same way; run by tests/test_ws_sizes.py
SANLAYOUT ?= $(SANDIR)/layout_walk
san_layout: $(SANOUT)
	mkdir -p $(dir $(SANLAYOUT))
	$(HIPCC) -std=c++17 --offload-arch=$(ARCH) --offload-host-only -x hip -O1 -g -fno-omit-frame-pointer -Wno-unused -I. \
	  -fsanitize=address,undefined,unsigned-integer-overflow -fno-sanitize-recover=undefined,unsigned-integer-overflow \
	  -c ../../tests/hip/layout_walk.cpp -o $(SANLAYOUT).o
	$(ROCM)/lib/llvm/bin/clang++ -fsanitize=address,undefined -shared-libsan $(SANLAYOUT).o -o $(SANLAYOUT) \
	  -L.. -lfthmc_hip_san -Wl,-rpath,$(abspath ..) -Wl,-rpath,$(dir $(SANRT))
