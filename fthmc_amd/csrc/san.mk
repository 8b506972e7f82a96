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

# The replica-exchange entry points (fthmc_ft_trajectory_pb_v, fthmc_hmc_trajectory_pb, fthmc_replica_swap, fthmc_ladder_init):
# tests/hip/tempering_walk.cpp as a stand-alone program against the host-side sanitizer build of the library (built first when it
# is missing or older than a source), the sanitizer runtimes linked in (nothing to preload), run by tests/test_tempering.py
SANTEMP ?= $(SANDIR)/tempering_walk
$(SANOUT): $(SRCS) common.h kernels.h integrator.h topo_int.h meta_tab.h api_call.h ../../include/fthmc_hip.h san.mk
	@$(MAKE) --no-print-directory -f san.mk san_build
san_tempering: $(SANOUT)
	mkdir -p $(dir $(SANTEMP))
	$(ROCM)/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan \
	  ../../tests/hip/tempering_walk.cpp -o $(SANTEMP) -L.. -lfthmc_hip_san -Wl,-rpath,$(abspath ..) -Wl,-rpath,$(dir $(SANRT))

# The Wilson-loop entry points (fthmc_wilson_loops_ws_bytes, fthmc_wilson_loops): tests/hip/loops_walk.cpp in the same way, run
# by tests/test_wilson_loops.py
SANLOOPS ?= $(SANDIR)/loops_walk
san_loops: $(SANOUT)
	mkdir -p $(dir $(SANLOOPS))
	$(ROCM)/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan \
	  ../../tests/hip/loops_walk.cpp -o $(SANLOOPS) -L.. -lfthmc_hip_san -Wl,-rpath,$(abspath ..) -Wl,-rpath,$(dir $(SANRT))

# The local-update entry point (fthmc_local_update): tests/hip/local_walk.cpp in the same way, run by tests/test_local_update.py
SANLOCAL ?= $(SANDIR)/local_walk
san_local: $(SANOUT)
	mkdir -p $(dir $(SANLOCAL))
	$(ROCM)/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan \
	  ../../tests/hip/local_walk.cpp -o $(SANLOCAL) -L.. -lfthmc_hip_san -Wl,-rpath,$(abspath ..) -Wl,-rpath,$(dir $(SANRT))

# The instanton-hit entry points (fthmc_instanton_hit, fthmc_instanton_ws_bytes) and the integer reductions of topo_int.h:
# tests/hip/instanton_walk.cpp in the same way, run by tests/test_instanton.py
SANINST ?= $(SANDIR)/instanton_walk
san_instanton: $(SANOUT)
	mkdir -p $(dir $(SANINST))
	$(ROCM)/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan \
	  ../../tests/hip/instanton_walk.cpp -o $(SANINST) -L.. -lfthmc_hip_san -Wl,-rpath,$(abspath ..) -Wl,-rpath,$(dir $(SANRT))

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

# The metadynamics entry points (fthmc_meta_ws_bytes, fthmc_meta_trajectory, fthmc_meta_deposit, fthmc_meta_force, fthmc_meta_action):
# tests/hip/meta_walk.cpp in the same way, run by tests/test_meta.py
SANMETA ?= $(SANDIR)/meta_walk
san_meta: $(SANOUT)
	mkdir -p $(dir $(SANMETA))
	$(ROCM)/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan \
	  ../../tests/hip/meta_walk.cpp -o $(SANMETA) -L.. -lfthmc_hip_san -Wl,-rpath,$(abspath ..) -Wl,-rpath,$(dir $(SANRT))

# The metadynamics-through-the-flow entry points (fthmc_ft_meta_ws_bytes, fthmc_ft_meta_trajectory_v, fthmc_ft_meta_force_v,
# fthmc_ft_meta_action_v): tests/hip/ft_meta_walk.cpp in the same way, run by tests/test_ft_meta.py
SANFTMETA ?= $(SANDIR)/ft_meta_walk
san_ft_meta: $(SANOUT)
	mkdir -p $(dir $(SANFTMETA))
	$(ROCM)/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan \
	  ../../tests/hip/ft_meta_walk.cpp -o $(SANFTMETA) -L.. -lfthmc_hip_san -Wl,-rpath,$(abspath ..) -Wl,-rpath,$(dir $(SANRT))
