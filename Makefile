# Builds the product library (gfx950 only) and the test oracle.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PKG := umi_collapse_rs_amd
CSRC := $(PKG)/csrc
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wextra -Wno-unused-parameter

LIB := $(PKG)/libumihip.so
OBJDIR := build/obj
# the library's translation units, listed once: the kernels (.hip), then the host side (.cpp)
SRCS := umihip_kernels umihip_seg umihip_collapse umihip_stage umihip_radix umihip_wide umihip_edit umihip_cr umihip_seq \
        umihip_consensus umihip_consensus_bam umihip_correct umihip_barcode umihip_count umihip_multigene umihip_stats umihip_cells umihip_genes umihip_gene_introns umihip_gene_classes umihip_gene_transcripts umihip_gene_transcript_classes umihip_velocity umihip_saturation umihip_junctions \
        umihip_api umihip_pipeline umihip_batch umihip_stage_api umihip_seq_api umihip_correct_api umihip_count_api umihip_genes_api umihip_cr_api umihip_data
OBJS := $(patsubst %,$(OBJDIR)/%.o,$(SRCS))
# development build (make dev): the shipped sources plus the round-1 tile kernels, their key sort
# and their options (-DUMIHIP_DEV), as libumihip_dev.so; the legacy cross-check tests load it
DEVDIR := build/obj_dev
DEVLIB := $(PKG)/libumihip_dev.so
DEVOBJS := $(patsubst %,$(DEVDIR)/%.o,$(SRCS)) $(DEVDIR)/umihip_legacy.o $(DEVDIR)/umihip_sort.o
HDRS := $(CSRC)/umihip_internal.h $(CSRC)/umihip_cons_group.h $(CSRC)/umihip_device.h $(CSRC)/umihip_plan.hpp $(CSRC)/umihip_io_layout.hpp $(CSRC)/umihip_host.hpp $(CSRC)/umihip_gene_index.hpp $(CSRC)/umihip_transcript_index.hpp $(CSRC)/umihip_junction_walk.hpp $(CSRC)/umihip_pair_table.h include/umihip.h
CLI := $(PKG)/bin/umicollapse

all: $(LIB) oracle cpptest primtest trtest jntest $(CLI)

# (the staging's host decisions: read by the staging unit alone)
$(OBJDIR)/umihip_stage.o $(DEVDIR)/umihip_stage.o: $(CSRC)/umihip_stage_plan.hpp

# one object per translation unit (the rocPRIM sort alone takes ~20 s to compile)
$(OBJDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c -o $@ -x hip $<

$(OBJDIR)/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c -o $@ -x hip $<

$(LIB): $(OBJS)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(OBJS) -ldl

$(DEVDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(DEVDIR)
	$(HIPCC) $(HIPFLAGS) -DUMIHIP_DEV -c -o $@ -x hip $<

$(DEVDIR)/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p $(DEVDIR)
	$(HIPCC) $(HIPFLAGS) -DUMIHIP_DEV -c -o $@ -x hip $<

$(DEVLIB): $(DEVOBJS)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(DEVOBJS) -ldl

dev: $(DEVLIB)

$(CLI): $(LIB) $(PKG)/host/umicollapse_main.cpp $(PKG)/host/cli.hpp $(PKG)/host/hiplib.hpp $(PKG)/host/staging.hpp $(PKG)/host/annotation.hpp \
        $(PKG)/host/two_pass.hpp $(PKG)/host/fastq_mode.hpp $(PKG)/host/bam.hpp $(PKG)/host/bgzf.hpp $(PKG)/host/fastq.hpp include/umihip.h
	mkdir -p $(PKG)/bin
	g++ -O2 -std=c++17 -Wall -Wextra -o $@ $(PKG)/host/umicollapse_main.cpp -lz -lpthread -ldl

cli: $(CLI)

oracle:
	$(MAKE) -s -C oracle

asm: $(CSRC)/umihip_kernels.hip $(HDRS)
	mkdir -p build
	$(HIPCC) $(HIPFLAGS) -S --cuda-device-only -o build/umihip_kernels.s -x hip $(CSRC)/umihip_kernels.hip \
	    -Rpass-analysis=kernel-resource-usage 2> build/resource_usage.txt || (cat build/resource_usage.txt; false)

cpptest: $(LIB) oracle tests/cpp/test_host.cpp $(PKG)/host/umi_collapse.hpp
	mkdir -p build
	g++ -O2 -std=c++17 -Wall -Wextra -o build/test_host tests/cpp/test_host.cpp \
	    -L$(PKG) -lumihip -Loracle -lumi_oracle -Wl,-rpath,'$$ORIGIN/../$(PKG)' -Wl,-rpath,'$$ORIGIN/../oracle'

# the sort and scan primitives on their own: umihip_radix.o and a program that calls it directly.  The
# test is compiled to an object first: on one line with -x hip the linker's object would be read as source
PRIMTEST := build/test_primitives
$(OBJDIR)/test_primitives.o: tests/cpp/test_primitives.hip tests/cpp/primitives_ref.hpp $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -c -o $@ -x hip $<

$(PRIMTEST): $(OBJDIR)/test_primitives.o $(OBJDIR)/umihip_radix.o
	$(HIPCC) $(HIPFLAGS) -o $@ $(OBJDIR)/test_primitives.o $(OBJDIR)/umihip_radix.o

primtest: $(PRIMTEST)

# the transcript index's lookup on the CPU, a program of its own (tests/test_transcript_index_cpu.py builds it once more, under sanitizers)
TRTEST := build/test_transcript_index
$(TRTEST): tests/cpp/test_transcript_index.cpp $(CSRC)/umihip_transcript_index.hpp $(CSRC)/umihip_gene_index.hpp
	@mkdir -p build
	g++ -O2 -std=c++17 -Wall -Wextra -o $@ tests/cpp/test_transcript_index.cpp

trtest: $(TRTEST)

# the junction walk on the CPU, a program of its own (tests/test_junction_model_cpu.py builds it once more, under sanitizers)
JNTEST := build/test_junction_walk
$(JNTEST): tests/cpp/test_junction_walk.cpp $(CSRC)/umihip_junction_walk.hpp
	@mkdir -p build
	g++ -O2 -std=c++17 -Wall -Wextra -o $@ tests/cpp/test_junction_walk.cpp

jntest: $(JNTEST)

clean:
	rm -f $(LIB) $(DEVLIB) $(CLI)
	rm -rf build
	$(MAKE) -s -C oracle clean

.PHONY: all dev oracle asm clean cpptest primtest trtest jntest cli
