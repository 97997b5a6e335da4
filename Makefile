# Top-level build. `make` builds everything in-tree (the .so files travel to the
# GPU box with the gpurun snapshot). gfx950 only.
HIPCC   ?= /opt/rocm/bin/hipcc
CLANGXX ?= /opt/rocm/llvm/bin/clang++
ARCH    ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -Wall -Wno-unused-function
CSRC := bdls_amd/csrc
LIB  := bdls_amd/lib

HDRS := $(wildcard $(CSRC)/*.h) include/bdls_hip.h

all: $(LIB)/libbdlship.so $(LIB)/libbdlsgen.so oracle tests/native/build/libhostsim.so \
     tests/native/build/libhostsim384.so tests/native/build/libhostsim384k.so \
     tests/native/build/libhostsim384s.so tests/native/build/libhostsim512.so \
     tests/native/build/libhostsimfused.so tests/native/build/libhostsim384c.so \
     tests/native/build/libhostsimlltab.so tests/native/build/libhostsim384i.so \
     tests/native/build/libhostsimhash.so $(LIB)/csp_load

$(LIB)/verify_kernels.o: $(CSRC)/verify_kernels.hip $(HDRS)
	@mkdir -p $(LIB)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# the P-384 pass (BH_CURVE_P384): a translation unit of its own
$(LIB)/verify384_kernels.o: $(CSRC)/verify384_kernels.hip $(HDRS)
	@mkdir -p $(LIB)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# the SHA-384 / SHA-512 digest pre-pass (BH_F_HASH_SHA384 / _SHA512): its own unit too
$(LIB)/sha512_kernels.o: $(CSRC)/sha512_kernels.hip $(HDRS)
	@mkdir -p $(LIB)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# bh_hash: SHA-256 / SHA3-256 over span records, digests or comparisons out: its own unit too
$(LIB)/hash_kernels.o: $(CSRC)/hash_kernels.hip $(HDRS)
	@mkdir -p $(LIB)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB)/bdls_hip.o: $(CSRC)/bdls_hip.cpp $(HDRS)
	@mkdir -p $(LIB)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB)/bdls_msg.o: $(CSRC)/bdls_msg.cpp include/bdls_hip.h
	@mkdir -p $(LIB)
	g++ -O2 -std=c++17 -fPIC -Wall -c $< -o $@

$(LIB)/fabric.o: $(CSRC)/fabric.cpp $(HDRS)
	@mkdir -p $(LIB)
	g++ -O2 -std=c++17 -fPIC -Wall -Wno-unknown-pragmas -c $< -o $@

$(LIB)/libbdlship.so: $(LIB)/verify_kernels.o $(LIB)/verify384_kernels.o $(LIB)/sha512_kernels.o \
                     $(LIB)/hash_kernels.o $(LIB)/bdls_hip.o $(LIB)/bdls_msg.o $(LIB)/fabric.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -lpthread

$(LIB)/libbdlsgen.so: bdls_amd/workload/gen.c
	@mkdir -p $(LIB)
	gcc -O2 -fPIC -shared -Wall -o $@ $< -lcrypto -lpthread

oracle:
	$(MAKE) -C oracle

# test-only host build of the device arithmetic (never linked into the product)
# (hostsim_prehashed.cpp includes hostsim.cpp and adds the prehashed BDLS entries)
tests/native/build/libhostsim.so: tests/native_prehashed/hostsim_prehashed.cpp \
                                  tests/native/hostsim.cpp $(HDRS)
	@mkdir -p tests/native/build
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -o $@ $< -lpthread

tests/native/build/libhostsim384.so: tests/native/hostsim384.cpp $(HDRS)
	@mkdir -p tests/native/build
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -o $@ $< -lpthread

# (hostsim384_keys.cpp includes hostsim384.cpp and adds the P-384 key registry's entries)
tests/native/build/libhostsim384k.so: tests/native_p384keys/hostsim384_keys.cpp \
                                      tests/native/hostsim384.cpp $(HDRS)
	@mkdir -p tests/native/build
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -o $@ $< -lpthread

# (hostsim384_seg.cpp includes hostsim384.cpp and adds the pass over two-span records)
tests/native/build/libhostsim384s.so: tests/native_p384seg/hostsim384_seg.cpp \
                                      tests/native/hostsim384.cpp $(HDRS)
	@mkdir -p tests/native/build
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -o $@ $< -lpthread

# (hostsim384_comb.cpp includes hostsim384.cpp and adds the per-pass key combs' entries)
tests/native/build/libhostsim384c.so: tests/native_p384comb/hostsim384_comb.cpp \
                                      tests/native/hostsim384.cpp $(HDRS)
	@mkdir -p tests/native/build
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -o $@ $< -lpthread

# (hostsim384_idx.cpp includes hostsim384.cpp and adds the index-keyed passes' entries and the
# packer at key width 96)
tests/native/build/libhostsim384i.so: tests/native_p384idx/hostsim384_idx.cpp \
                                      tests/native/hostsim384.cpp $(HDRS)
	@mkdir -p tests/native/build
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -o $@ $< -lpthread

# stand-alone sanitizer run of the index-keyed prep and grouping on the CPU
# (tests/test_p384_batch_cpu.py builds and runs it)
tests/native/build/idx384_selftest: tests/native_p384idx/hostsim384_idx.cpp \
                                    tests/native/hostsim384.cpp $(HDRS)
	@mkdir -p tests/native/build
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	  -DIDX384_SELFTEST_MAIN -o $@ $< -lcrypto -lpthread

tests/native/build/libhostsim512.so: tests/native_sha512/hostsim_sha512.cpp $(HDRS)
	@mkdir -p tests/native/build
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -o $@ $<

# hashspan.h's span loaders and compare step (bh_hash's kernels) on their own
tests/native/build/libhostsimhash.so: tests/native_hash/hostsim_hash.cpp $(HDRS)
	@mkdir -p tests/native/build
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -o $@ $<

# the fused field / point formulas (f_mul2, j_zaddc, the composite 2A + T) on their own
tests/native/build/libhostsimfused.so: tests/native_fused/hostsim_fused.cpp $(HDRS)
	@mkdir -p tests/native/build
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -o $@ $<

# the per-batch comb table build (lltab_build) and j_dbl on their own
tests/native/build/libhostsimlltab.so: tests/native_lltab/hostsim_lltab.cpp $(HDRS)
	@mkdir -p tests/native/build
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -o $@ $<

# stand-alone sanitizer run of lltab_build's scratch layout on the CPU
# (tests/test_lltab_cpu.py builds and runs it)
tests/native/build/lltab_selftest: tests/native_lltab/lltab_selftest.cpp \
                                   tests/native_lltab/hostsim_lltab.cpp $(HDRS)
	@mkdir -p tests/native/build
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	  -o $@ $<

# stand-alone sanitizer run of sha512.h on the CPU (tests/test_sha2wide_cpu.py builds and runs it)
tests/native/build/sha512_selftest: tests/native_sha512/sha512_selftest.cpp $(HDRS)
	@mkdir -p tests/native/build
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	  -o $@ $< -lcrypto

# stand-alone sanitizer run of comb384.h on the CPU (tests/test_p384_comb_cpu.py builds and runs it)
tests/native/build/comb384_selftest: tests/native_p384comb/comb384_selftest.cpp \
                                     tests/native_p384comb/hostsim384_comb.cpp \
                                     tests/native/hostsim384.cpp $(HDRS)
	@mkdir -p tests/native/build
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	  -o $@ $< -lcrypto -lpthread

# build-kernel experiments (profiles/r02/exp_build): not part of `all`
EXP_VARIANTS := base:
exp:
	@mkdir -p build/exp
	@for v in $(EXP_VARIANTS); do n=$${v%%:*}; f=$$(echo $${v#*:} | tr '+' ' '); \
	  $(HIPCC) $(HIPFLAGS) $$f -c $(CSRC)/verify_kernels.hip -o build/exp/vk_$$n.o && \
	  $(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o build/exp/libbdlship_$$n.so build/exp/vk_$$n.o \
	    $(LIB)/verify384_kernels.o $(LIB)/sha512_kernels.o $(LIB)/hash_kernels.o $(LIB)/bdls_hip.o \
    $(LIB)/bdls_msg.o \
	    $(LIB)/fabric.o -lpthread || exit 1; done

clean:
	rm -rf $(LIB) tests/native/build
	$(MAKE) -C oracle clean

.PHONY: all oracle clean

$(LIB)/ubench: $(CSRC)/ubench.hip $(HDRS)
	@mkdir -p $(LIB)
	$(HIPCC) $(HIPFLAGS) -o $@ $<
all: $(LIB)/ubench

# native load generator for the coalesced single Verify (bench.py side configs)
$(LIB)/csp_load: tools/csp_load.cpp include/bdls_hip.h $(LIB)/libbdlship.so
	g++ -O2 -std=c++17 -Wall -o $@ $< -L$(LIB) -lbdlship -Wl,-rpath,'$$ORIGIN' -lpthread
