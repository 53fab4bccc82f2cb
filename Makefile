# Build of the MI355X block-hash path (gfx950 only) and of the CPU oracle.
#   make            -> ciruela_amd/libciruela_amd.so, bin/ciruela-index, the two
#                      load drivers under build/, oracle
#   make oracle     -> oracle/build/liboracle_blake2b.so (test infrastructure)
#   make sketch_fuzz -> build/sketch_fuzz (the sketch rule under ASan + UBSan; not in `all`)
#   make emit_fuzz  -> build/emit_fuzz (the emit rule under ASan + UBSan; not in `all`)
#   make scatter_fuzz -> build/scatter_fuzz (the scatter rule under ASan + UBSan; not in `all`)
#   make gather_fuzz -> build/gather_fuzz (the gather rule under ASan + UBSan; not in `all`)
#   make copyblk_fuzz -> build/copyblk_fuzz (the copy and plan rules under ASan + UBSan; not in `all`)
#   make update_fuzz -> build/update_fuzz (the in-place update rule under ASan + UBSan; not in
#                      `all`, built by `make sanitizers`)
#   make asan/tsan  -> build/host_{asan,tsan}_driver (host code under the
#                      sanitizers; `make sanitizers` = both; not in `all`)
HIPCC ?= /opt/rocm/bin/hipcc
CXX ?= g++
CC ?= gcc
ARCH ?= gfx950
# COV5 keeps the code object loadable by the ROCm 7.0 runtime that ships
# inside the PyTorch wheel as well as by /opt/rocm (7.2).
COMMON := -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -Iinclude -Iciruela_amd/csrc
HIPFLAGS ?= $(COMMON) --offload-arch=$(ARCH) -mcode-object-version=5
HOSTFLAGS ?= $(COMMON) -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
CSRC := ciruela_amd/csrc
OBJDIR := build/obj
LIB := ciruela_amd/libciruela_amd.so
CLI := bin/ciruela-index

SRCS_HIP := $(CSRC)/kernels.hip $(CSRC)/order.hip $(CSRC)/join.hip \
            $(CSRC)/idxscan.hip $(CSRC)/extents.hip $(CSRC)/repeats.hip \
            $(CSRC)/files.hip $(CSRC)/plan.hip $(CSRC)/sketch.hip $(CSRC)/emit.hip \
            $(CSRC)/scatter.hip $(CSRC)/gather.hip $(CSRC)/copyblk.hip $(CSRC)/update.hip
SRCS_CPP := $(CSRC)/runtime.cpp $(CSRC)/dirsig.cpp $(CSRC)/scan.cpp $(CSRC)/check.cpp \
            $(CSRC)/links.cpp $(CSRC)/sources.cpp $(CSRC)/repeats.cpp $(CSRC)/idxscan.cpp \
            $(CSRC)/files.cpp $(CSRC)/copies.cpp $(CSRC)/plan.cpp $(CSRC)/sketch.cpp $(CSRC)/memindex.cpp $(CSRC)/store.cpp $(CSRC)/reload.cpp $(CSRC)/update.cpp $(CSRC)/devcall.cpp $(CSRC)/registry.cpp $(CSRC)/blake2b_host.cpp \
            $(CSRC)/sha512_host.cpp
OBJS := $(patsubst $(CSRC)/%.hip,$(OBJDIR)/%.hip.o,$(SRCS_HIP)) \
        $(patsubst $(CSRC)/%.cpp,$(OBJDIR)/%.o,$(SRCS_CPP))
HDRS := $(wildcard $(CSRC)/*.hpp) include/ciruela_blockhash.h

all: $(LIB) $(CLI) build/hash_bytes_conc build/verify_daemon_sim oracle

# (x.hip -> x.hip.o: idxscan.hip and idxscan.cpp share a stem)
$(OBJDIR)/%.hip.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# host-only translation units: compiled by hipcc as C++ (HIP headers, no device code)
$(OBJDIR)/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HOSTFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(OBJS) -lpthread

$(CLI): $(CSRC)/cli.cpp $(LIB) $(HDRS)
	@mkdir -p bin
	$(HIPCC) $(HOSTFLAGS) $< -o $@ -Lciruela_amd -lciruela_amd \
	    -Wl,-rpath,'$$ORIGIN/../ciruela_amd'

# concurrent hash_bytes callers from C threads (tools/hash_bytes_conc.cpp)
build/hash_bytes_conc: tools/hash_bytes_conc.cpp $(LIB) include/ciruela_blockhash.h
	@mkdir -p build
	$(HIPCC) $(HOSTFLAGS) $< -o $@ -Lciruela_amd -lciruela_amd \
	    -Wl,-rpath,'$$ORIGIN/../ciruela_amd' -lpthread

# the daemon's per-block verify under load (tools/verify_daemon_sim.cpp)
build/verify_daemon_sim: tools/verify_daemon_sim.cpp $(LIB) include/ciruela_blockhash.h
	@mkdir -p build
	$(HIPCC) $(HOSTFLAGS) $< -o $@ -Lciruela_amd -lciruela_amd \
	    -Wl,-rpath,'$$ORIGIN/../ciruela_amd' -lpthread

# the library's host code under ASan + UBSan against the production device
# code (tools/host_asan_driver.cpp; sanitizers on the host side only)
ASAN_HOST := -O1 -g -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
             -Xarch_host -fno-sanitize-recover=all -Xarch_host -fno-omit-frame-pointer
ASAN_OBJS := $(patsubst $(CSRC)/%.hip,$(OBJDIR)/%.hip.o,$(SRCS_HIP)) \
             $(patsubst $(CSRC)/%.cpp,build/asan/%.o,$(SRCS_CPP)) build/asan/host_asan_driver.o
build/asan/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p build/asan
	$(HIPCC) $(HOSTFLAGS) $(ASAN_HOST) -c $< -o $@
build/asan/host_asan_driver.o: tools/host_asan_driver.cpp include/ciruela_blockhash.h
	@mkdir -p build/asan
	$(HIPCC) $(HOSTFLAGS) $(ASAN_HOST) -c $< -o $@
build/host_asan_driver: $(ASAN_OBJS)
	$(HIPCC) $(HIPFLAGS) $(ASAN_HOST) -o $@ $(ASAN_OBJS) -lpthread
asan: build/host_asan_driver

# the same driver with the host code under ThreadSanitizer
# (TSAN_OPTIONS=suppressions=tools/tsan_hip.supp)
TSAN_HOST := -O1 -g -Xarch_host -fsanitize=thread
TSAN_OBJS := $(patsubst $(CSRC)/%.hip,$(OBJDIR)/%.hip.o,$(SRCS_HIP)) \
             $(patsubst $(CSRC)/%.cpp,build/tsan/%.o,$(SRCS_CPP)) build/tsan/host_asan_driver.o
build/tsan/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p build/tsan
	$(HIPCC) $(HOSTFLAGS) $(TSAN_HOST) -c $< -o $@
build/tsan/host_asan_driver.o: tools/host_asan_driver.cpp include/ciruela_blockhash.h
	@mkdir -p build/tsan
	$(HIPCC) $(HOSTFLAGS) $(TSAN_HOST) -c $< -o $@
build/host_tsan_driver: $(TSAN_OBJS)
	$(HIPCC) $(HIPFLAGS) $(TSAN_HOST) -o $@ $(TSAN_OBJS) -lpthread
tsan: build/host_tsan_driver

sanitizers: asan tsan update_fuzz

# the sketch rule (sketch.hpp) and the index parser under ASan + UBSan: a
# stand-alone host program (tools/sketch_fuzz.cpp), no device code
build/sketch_fuzz: tools/sketch_fuzz.cpp $(CSRC)/sketch.hpp $(CSRC)/dirsig.hpp $(CSRC)/dirsig.cpp
	@mkdir -p build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
	    -I$(CSRC) tools/sketch_fuzz.cpp $(CSRC)/dirsig.cpp -o $@
sketch_fuzz: build/sketch_fuzz

# the emit rule (emit.hpp) under ASan + UBSan: a stand-alone host program
# (tools/emit_fuzz.cpp), no device code
build/emit_fuzz: tools/emit_fuzz.cpp $(CSRC)/emit.hpp $(CSRC)/dirsig.hpp $(CSRC)/dirsig.cpp
	@mkdir -p build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
	    -I$(CSRC) tools/emit_fuzz.cpp $(CSRC)/dirsig.cpp -o $@
emit_fuzz: build/emit_fuzz

# the scatter rule (scatter.hpp) over pack.hpp's runs under ASan + UBSan: a
# stand-alone host program (tools/scatter_fuzz.cpp), no device code
build/scatter_fuzz: tools/scatter_fuzz.cpp $(CSRC)/scatter.hpp $(CSRC)/pack.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
	    -I$(CSRC) tools/scatter_fuzz.cpp -o $@
scatter_fuzz: build/scatter_fuzz

# the gather rule (gather.hpp; the kernel is gather.hip) over pack.hpp's runs under
# ASan + UBSan: a stand-alone host program (tools/gather_fuzz.cpp), no device code
build/gather_fuzz: tools/gather_fuzz.cpp $(CSRC)/gather.hpp $(CSRC)/scatter.hpp $(CSRC)/pack.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
	    -I$(CSRC) tools/gather_fuzz.cpp -o $@
gather_fuzz: build/gather_fuzz

# the copy and plan rules (copyblk.hpp; the kernels are copyblk.hip) under ASan + UBSan:
# a stand-alone host program (tools/copyblk_fuzz.cpp), no device code
build/copyblk_fuzz: tools/copyblk_fuzz.cpp $(CSRC)/copyblk.hpp $(CSRC)/scatter.hpp $(CSRC)/pack.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
	    -I$(CSRC) tools/copyblk_fuzz.cpp -o $@
copyblk_fuzz: build/copyblk_fuzz

# the in-place update rule (update.hpp over copyblk.hpp; the kernels are update.hip) under
# ASan + UBSan: a stand-alone host program (tools/update_fuzz.cpp), no device code
build/update_fuzz: tools/update_fuzz.cpp $(CSRC)/update.hpp $(CSRC)/copyblk.hpp $(CSRC)/scatter.hpp $(CSRC)/pack.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
	    -I$(CSRC) tools/update_fuzz.cpp -o $@
update_fuzz: build/update_fuzz

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf build $(LIB) $(CLI)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean asan tsan sanitizers sketch_fuzz emit_fuzz scatter_fuzz gather_fuzz copyblk_fuzz update_fuzz
