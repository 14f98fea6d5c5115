# Build libchunkio_amd.so (HIP kernels for gfx950 + C ABI) and the oracle.
# `python -c "import __graft_entry__ as g; g.build()"` drives this file.

HIPCC   ?= /opt/rocm/bin/hipcc
CC      ?= gcc
CXX     ?= g++
ARCH    ?= gfx950
OUT     := chunkio_amd/lib
LIB     := $(OUT)/libchunkio_amd.so
SRC     := chunkio_amd/csrc
BLD     := build
INC     := -Iinclude -I$(SRC)

CFLAGS   := -O3 -fPIC -Wall -Wextra -std=gnu11 $(INC)
# crc_plan.cpp is plain C++: no offload arch and no ROCm include directory, so
# a HIP header there fails the build.
CXXFLAGS := -O3 -fPIC -Wall -Wextra -std=c++17 $(INC)
HIPFLAGS := -O3 -fPIC --offload-arch=$(ARCH) -std=c++17 -Wall $(INC) -munsafe-fp-atomics \
            -mllvm -amdgpu-atomic-optimizer-strategy=None -mllvm -amdgpu-kernarg-preload-count=9

COBJS   := $(BLD)/host_copy.o $(BLD)/crc32_host.o $(BLD)/crc32_scalar.o $(BLD)/cio_verify.o $(BLD)/cio_sync.o $(BLD)/cioa_chunk.o $(BLD)/crc_route.o $(BLD)/crc_cpu_batch.o $(BLD)/cio_sha1.o
HOBJS   := $(BLD)/crc32_gpu.o $(BLD)/probe_gpu.o $(BLD)/gpu_runtime.o $(BLD)/crc_plan.o $(BLD)/host_pipeline.o $(BLD)/sha1_gpu.o $(BLD)/devplan_gpu.o $(BLD)/write_dev_gpu.o $(BLD)/read_dev_gpu.o $(BLD)/write_records_gpu.o $(BLD)/sort_records_gpu.o $(BLD)/grow_dev_gpu.o $(BLD)/rotate_dev_gpu.o $(BLD)/tx_dev_gpu.o $(BLD)/pool_dev_gpu.o $(BLD)/pool_set_gpu.o $(BLD)/coalesce_gpu.o $(BLD)/alloc_set_gpu.o $(BLD)/persist_host.o $(BLD)/route_gpu.o

CTEST   := tests/c/bin
REF_INC := /root/reference/include/chunkio/cio_crc32.h
REF_SHA1 := /root/reference/src/cio_sha1.c
CTESTS  := $(CTEST)/test_crc32_dropin $(CTEST)/test_chunk_api $(CTEST)/test_multi $(CTEST)/test_sha1 \
           $(if $(wildcard $(REF_INC)),$(CTEST)/test_crc32_dropin_ref) $(if $(wildcard $(REF_SHA1)),$(CTEST)/test_sha1_ref)
CLINK   := -Lchunkio_amd/lib -lchunkio_amd -Wl,-rpath,'$$ORIGIN/../../../chunkio_amd/lib'

all: $(LIB) oracle ctests

# C callers of the public headers (tests/test_c_api.py runs them).  The _ref
# variant compiles the reference's own include/chunkio/cio_crc32.h, unmodified,
# against include/crc32/crc32.h (only where /root/reference exists).
ctests: $(CTESTS)

$(CTEST)/test_crc32_dropin: tests/c/test_crc32_dropin.c $(LIB) include/crc32/crc32.h
	@mkdir -p $(CTEST)
	$(CC) -O2 -Wall -Wextra -std=gnu11 -Iinclude -o $@ $< $(CLINK)

$(CTEST)/test_crc32_dropin_ref: tests/c/test_crc32_dropin.c $(LIB) include/crc32/crc32.h
	@mkdir -p $(CTEST)
	$(CC) -O2 -Wall -Wextra -std=gnu11 -DCIOA_REF_BOUNDARY -Iinclude -I/root/reference/include -o $@ $< $(CLINK)

# chunkio's cio_sha1 API: the library's exports, and the reference's own
# cio_sha1.h + cio_sha1.c (unmodified, compiled where they lie) over
# include/sha1/sha1.h -- include/ ahead of the reference's include/.
$(CTEST)/test_sha1: tests/c/test_sha1.c $(LIB) include/sha1/sha1.h include/chunkio_amd/cio_sha1.h
	@mkdir -p $(CTEST)
	$(CC) -O2 -Wall -Wextra -std=gnu11 -Iinclude -o $@ $< $(CLINK)

$(CTEST)/test_sha1_ref: tests/c/test_sha1.c $(REF_SHA1) $(LIB) include/sha1/sha1.h
	@mkdir -p $(CTEST)
	$(CC) -O2 -Wall -std=gnu11 -DCIOA_REF_BOUNDARY -Iinclude -I/root/reference/include -o $@ $< $(REF_SHA1) $(CLINK)

$(CTEST)/test_chunk_api: tests/c/test_chunk_api.c $(LIB) $(wildcard include/*/*.h)
	@mkdir -p $(CTEST)
	$(CC) -O2 -Wall -Wextra -std=gnu11 -Iinclude -o $@ $< $(CLINK)

$(CTEST)/test_multi: tests/c/test_multi.c $(LIB) include/chunkio_amd/cio_crc32_gpu.h
	@mkdir -p $(CTEST)
	$(CC) -O2 -Wall -Wextra -std=gnu11 -Iinclude -o $@ $< $(CLINK) -lpthread

$(BLD)/%.o: $(SRC)/%.c $(wildcard $(SRC)/*.h) $(wildcard include/*/*.h)
	@mkdir -p $(BLD)
	$(CC) $(CFLAGS) -c -o $@ $<

$(BLD)/%.o: $(SRC)/%.cpp $(wildcard $(SRC)/*.h) $(wildcard include/*/*.h)
	@mkdir -p $(BLD)
	$(CXX) $(CXXFLAGS) -c -o $@ $<

$(BLD)/%.o: $(SRC)/%.hip $(wildcard $(SRC)/*.h) $(wildcard include/*/*.h)
	@mkdir -p $(BLD)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(LIB): $(COBJS) $(HOBJS)
	@mkdir -p $(OUT)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $^ -lpthread

oracle:
	$(MAKE) -C oracle

# A/B variant of the library: make ablib VAR=name DEFS="-DFOO" -> chunkio_amd/lib/ab/name.so
# $(DEFS) reaches every unit that reads cio_diag.h for CRC: the kernels, the
# planner (CIO_HEAD_ALIGN in plan_build) and the runtime (cio_gpu_version).
# Every other object is the shipped library's.
ABOBJS  := crc32_gpu gpu_runtime crc_plan
ablib:
	@mkdir -p $(OUT)/ab $(BLD)/ab
	$(HIPCC) $(HIPFLAGS) $(DEFS) -c -o $(BLD)/ab/crc32_gpu_$(VAR).o $(SRC)/crc32_gpu.hip
	$(HIPCC) $(HIPFLAGS) $(DEFS) -c -o $(BLD)/ab/gpu_runtime_$(VAR).o $(SRC)/gpu_runtime.hip
	$(CXX) $(CXXFLAGS) $(DEFS) -c -o $(BLD)/ab/crc_plan_$(VAR).o $(SRC)/crc_plan.cpp
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $(OUT)/ab/$(VAR).so $(COBJS) $(ABOBJS:%=$(BLD)/ab/%_$(VAR).o) $(filter-out $(ABOBJS:%=$(BLD)/%.o),$(HOBJS)) -lpthread

# Same for the SHA-1 kernel: make ablib_sha1 VAR=name DEFS="-DCIO_SHA1_CHAINS=32"
ablib_sha1:
	@mkdir -p $(OUT)/ab $(BLD)/ab
	$(HIPCC) $(HIPFLAGS) $(DEFS) -c -o $(BLD)/ab/sha1_gpu_$(VAR).o $(SRC)/sha1_gpu.hip
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $(OUT)/ab/$(VAR).so $(COBJS) $(BLD)/ab/sha1_gpu_$(VAR).o $(filter-out $(BLD)/sha1_gpu.o,$(HOBJS)) -lpthread

# The device assembly, for a diff against the parent's: `make asmall` every
# .hip unit, `make asm` the CRC kernels and the probes, `make asmset` the units
# of the pool set's coalescing.
asmall: $(patsubst $(SRC)/%.hip,$(BLD)/asm/%.s,$(wildcard $(SRC)/*.hip))
asm: $(BLD)/asm/crc32_gpu.s $(BLD)/asm/probe_gpu.s
asmset: $(BLD)/asm/sort_records_gpu.s $(BLD)/asm/pool_set_gpu.s $(BLD)/asm/coalesce_gpu.s

$(BLD)/asm/%.s: $(SRC)/%.hip $(wildcard $(SRC)/*.h) $(wildcard include/*/*.h)
	@mkdir -p $(BLD)/asm
	$(HIPCC) $(HIPFLAGS) --offload-device-only -S -o $@ $<

# The host checks: the HIP-free headers under csrc/ -- the text the device
# kernels run -- under ASan + UBSan, each from a stand-alone program (no GPU,
# no HIP): `make <name>check` builds tools/<program>.cpp and runs it.
#   plancheck      the host planner: the shipped choices over the geometries of
#                  tests/test_plan_choice.py (with crc_plan.cpp and crc32_host.c)
#   copycheck      write_dev_copy.h: the append copy's partition and unit arithmetic
#   movecheck      write_dev_move.h: the in-place move's partition, save / shift
#                  split and tiles, the segments of each kernel in three orders
#   placecheck     read_dev_place.h: the read path's header, scan and place
#                  kernels workgroup by workgroup in three orders, against a
#                  sequential sum
#   recordscheck   write_dev_records.h: the grouped append's segmented scan and
#                  acceptance, in three orders, against a sequential loop per image
#   sortcheck      sort_records.h: the stable radix sort's histogram, scan and
#                  scatter in three orders and wave by wave with the ballot
#                  emulated over 64 lanes, against std::stable_sort
#   growcheck      grow_dev.h: the header, scan, place and commit kernels in three
#                  orders against a sequential loop in 128-bit arithmetic, and the
#                  zero fill lane by lane over buffers of exactly the batch's extent
#   rotatecheck    rotate_dev.h: the same for rotate, and the sums' wave-level
#                  pre-reduction lane by lane against a sequential sum
#   txcheck        tx_dev.h: begin, rollback (plain and the chain's header and
#                  commit steps) and commit in three orders over real image bytes
#                  in buffers of exactly the batch's extent, against a sequential
#                  loop, and the condition kernel wave by wave over 64 explicit
#                  lanes with a count of the atomics issued
#   poolcheck      pool_dev.h: the release's kernels and the pool-aware rotate's
#                  place and commit in three orders against a sequential loop in
#                  128-bit arithmetic, the arrays of exactly the batch's extent
#   poolsetcheck   pool_set.h: the release into the set and the grow out of it in
#                  three orders and wave by wave with the ballots emulated over 64
#                  lanes, against a sequential loop in 128-bit arithmetic
#   coalescecheck  coalesce.h: the whole chain in three orders and wave by wave,
#                  the sort as sort_records.h's passes, against a sequential loop
#                  in 128-bit arithmetic, the arrays of exactly the set's extent
#   imagecheck     image_dev.h: the image check at every boundary of its rules
#                  over buffers of exactly the image's extent, and with a null
#                  base where no byte may be read
#   alloccheck     alloc_set.h: the allocation out of the set, entry by entry at
#                  every boundary of its rules and whole batches against a
#                  sequential loop in 128-bit arithmetic, the set's arrays of
#                  exactly the set's extent
#   persistcheck   persist_plan.h: the round planner and the file-size rule at
#                  every boundary, against a restatement in 128-bit arithmetic
#   routecheck     route.h: the tag rule at every boundary, and the lower bound,
#                  the candidates' walk and the choice over sorted arrays, shuffled
#                  arrays, arrays with entries >= n, all-equal keys and the keys 0
#                  and 0xffffffff, the arrays of exactly n entries, against a
#                  linear restatement
SANFLAGS := -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
CHECKS   := plan copy move place records sort grow rotate tx pool pool_set coalesce image alloc persist route
CHECKTGT := $(foreach c,$(CHECKS),$(subst _,,$(c))check)

# plan_check links the planner and the host CRC it calls.
plan_CHECK_LINK := $(SRC)/crc_plan.cpp $(BLD)/plancheck/crc32_host.o -lpthread
$(BLD)/plancheck/crc32_host.o: $(SRC)/crc32_host.c $(wildcard $(SRC)/*.h) $(wildcard include/*/*.h)
	@mkdir -p $(BLD)/plancheck
	$(CC) $(SANFLAGS) -std=gnu11 $(INC) -c -o $@ $<

# $(1): the program's name without _check, $(2): the target
define CHECK_RULE
$(2): $$(filter %.o,$$($(1)_CHECK_LINK))
	@mkdir -p $(BLD)/$(2)
	$(CXX) $(SANFLAGS) -Wall -Wextra -std=c++17 $(INC) -o $(BLD)/$(2)/$(1)_check tools/$(1)_check.cpp $$($(1)_CHECK_LINK)
	$(BLD)/$(2)/$(1)_check
endef
$(foreach c,$(CHECKS),$(eval $(call CHECK_RULE,$(c),$(subst _,,$(c))check)))

# make install PREFIX=/usr/local: the library, the public headers (crc32/crc32.h,
# sha1/sha1.h, chunkio_amd/*.h) and a pkg-config file, for a chunkio build to
# link against.
PREFIX ?= /usr/local
install: $(LIB)
	install -d $(DESTDIR)$(PREFIX)/lib/pkgconfig $(DESTDIR)$(PREFIX)/include/crc32 \
	    $(DESTDIR)$(PREFIX)/include/sha1 $(DESTDIR)$(PREFIX)/include/chunkio_amd
	install -m 755 $(LIB) $(DESTDIR)$(PREFIX)/lib/
	install -m 644 include/crc32/crc32.h $(DESTDIR)$(PREFIX)/include/crc32/
	install -m 644 include/sha1/sha1.h $(DESTDIR)$(PREFIX)/include/sha1/
	install -m 644 include/chunkio_amd/*.h $(DESTDIR)$(PREFIX)/include/chunkio_amd/
	printf 'prefix=%s\nlibdir=$${prefix}/lib\nincludedir=$${prefix}/include\n\nName: chunkio_amd\nDescription: MI355X-native CRC-32 / SHA-1 path of fluent/chunkio (drop-in crc32.h, batched GPU calls)\nVersion: 0.5.0\nLibs: -L$${libdir} -lchunkio_amd\nCflags: -I$${includedir}\n' \
	    "$(PREFIX)" > $(DESTDIR)$(PREFIX)/lib/pkgconfig/chunkio_amd.pc

clean:
	rm -rf $(BLD) $(LIB) $(CTEST)
	$(MAKE) -C oracle clean

.PHONY: all oracle asm asmall asmset clean ctests ablib ablib_sha1 $(CHECKTGT) install
