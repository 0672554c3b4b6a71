# Builds the C-ABI shared library of the hot path for gfx950 (MI355X), in-tree.
#   make -j8        -> g_adaptivity_amd/libgadapt_hip.so   (one object per kernel family: csrc/gadapt_internal.h)
#                      g_adaptivity_amd/libgadapt_fem.so   (the FEM tails: 2-D pde_loss and 1-D Burgers / Poisson; fem_csrc/, include/gadapt_fem.h)
#                      g_adaptivity_amd/libgadapt_mesh.so  (batched MMPDE5 and Monge-Ampere target meshes; mesh_csrc/, include/gadapt_mesh.h)
#   make resources  -> per-kernel VGPR/SGPR/LDS/occupancy report
#   make DEV_C=64   -> development build: tiled kernels for one hidden size only (never shipped)
HIPCC      ?= /opt/rocm/bin/hipcc
ARCH       ?= gfx950
CSRC       := g_adaptivity_amd/csrc
OBJDIR     := build/obj
LIB        := g_adaptivity_amd/libgadapt_hip.so
FEM_CSRC   := g_adaptivity_amd/fem_csrc
FEM_LIB    := g_adaptivity_amd/libgadapt_fem.so
FEM_OBJS   := $(OBJDIR)/fem_kernels.o $(OBJDIR)/fem1d_kernels.o $(OBJDIR)/spline_kernels.o $(OBJDIR)/descent_kernels.o $(OBJDIR)/fem_topology.o
MESH_CSRC  := g_adaptivity_amd/mesh_csrc
MESH_LIB   := g_adaptivity_amd/libgadapt_mesh.so
HIPFLAGS   := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Iinclude -I$(CSRC) -Wall -Wno-unused-variable -Wno-unused-but-set-variable -Wno-unused-function $(EXTRA)
ifdef DEV_C
HIPFLAGS   += -DGADAPT_DEV_C=$(DEV_C)
endif
UNITS      := gadapt_kernels gadapt_tu_fwd gadapt_tu_bwd_target gadapt_tu_bwd_source gadapt_tu_smallmesh gadapt_tu_sparse gadapt_tu_gat gadapt_tu_cnn
OBJS       := $(UNITS:%=$(OBJDIR)/%.o) $(OBJDIR)/csr_build.o
SHARED     := $(CSRC)/gadapt_internal.h $(CSRC)/gadapt_common.inc $(CSRC)/gadapt_block_plan.h $(CSRC)/gadapt_narrow_plan.h include/gadapt_hip.h
TAIL_PLAN  := $(CSRC)/gadapt_tail_plan.h

all: $(LIB) $(FEM_LIB) $(MESH_LIB)

# the differentiable P1 FEM tail of loss_type='pde_loss' (include/gadapt_fem.h): its own library, built without FMA contraction
# (fem_csrc/fem_common.h: the reference's edge tests compare rounded sums)
$(FEM_LIB): $(FEM_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(FEM_OBJS)

$(OBJDIR)/fem_kernels.o: $(FEM_CSRC)/fem_kernels.hip $(FEM_CSRC)/fem_window_kernels.hip $(FEM_CSRC)/fem_window_grad_kernels.hip $(FEM_CSRC)/fem_wave_grad_kernels.hip $(FEM_CSRC)/fem_wave_fwd_kernels.hip $(FEM_CSRC)/fem_common.h $(FEM_CSRC)/fem_host.h include/gadapt_fem.h
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c -o $@ $<

$(OBJDIR)/fem1d_kernels.o: $(FEM_CSRC)/fem1d_kernels.hip $(FEM_CSRC)/fem_common.h $(FEM_CSRC)/fem1d_common.h $(FEM_CSRC)/fem_host.h include/gadapt_fem.h
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c -o $@ $<

$(OBJDIR)/spline_kernels.o: $(FEM_CSRC)/spline_kernels.hip $(FEM_CSRC)/fem1d_common.h $(FEM_CSRC)/fem_host.h include/gadapt_fem.h
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c -o $@ $<

$(OBJDIR)/descent_kernels.o: $(FEM_CSRC)/descent_kernels.hip $(FEM_CSRC)/fem_common.h $(FEM_CSRC)/fem1d_common.h $(FEM_CSRC)/fem_host.h include/gadapt_fem.h
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c -o $@ $<

$(OBJDIR)/fem_topology.o: $(FEM_CSRC)/fem_topology.cpp include/gadapt_fem.h
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c -o $@ $<

# the MMPDE5 target-mesh generator (include/gadapt_mesh.h): its own library, without FMA contraction like the FEM tails
# (the stopping step of the fp32 iteration follows the rounding of its increments)
MESH_OBJS  := $(OBJDIR)/mmpde5_kernels.o $(OBJDIR)/ma_kernels.o $(OBJDIR)/ma_strided_kernels.o $(OBJDIR)/ma_m2n_slow_kernels.o \
              $(OBJDIR)/ma_table_kernels.o
$(MESH_LIB): $(MESH_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(MESH_OBJS)

$(OBJDIR)/mmpde5_kernels.o: $(MESH_CSRC)/mmpde5_kernels.hip $(MESH_CSRC)/mesh_common.h include/gadapt_mesh.h
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c -o $@ $<

# the Monge-Ampere target meshes (2-D): the same library and the same flags; the iteration and the batch check stated once
MA_SHARED  := $(MESH_CSRC)/ma_iteration.h $(MESH_CSRC)/ma_host.h $(MESH_CSRC)/mesh_common.h include/gadapt_mesh.h
$(OBJDIR)/ma_kernels.o: $(MESH_CSRC)/ma_kernels.hip $(MA_SHARED)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c -o $@ $<

# their strided route with an fp64 potential (up to 81 x 81): an object of its own, the same flags
$(OBJDIR)/ma_strided_kernels.o: $(MESH_CSRC)/ma_strided_kernels.hip $(MA_SHARED)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c -o $@ $<

# the M2N 'slow' monitor (a P1 Poisson solve on the moving mesh inside the update loop, up to 24 x 24): the same flags
$(OBJDIR)/ma_m2n_slow_kernels.o: $(MESH_CSRC)/ma_m2n_slow_kernels.hip $(MA_SHARED)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c -o $@ $<

# Monge-Ampere meshes from a tabulated monitor, both routes: the same flags
$(OBJDIR)/ma_table_kernels.o: $(MESH_CSRC)/ma_table_kernels.hip $(MA_SHARED)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c -o $@ $<

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

$(OBJDIR)/gadapt_kernels.o: $(CSRC)/gadapt_small.inc $(TAIL_PLAN)
$(OBJDIR)/gadapt_tu_fwd.o: $(CSRC)/gadapt_fwd.inc $(CSRC)/gadapt_wide.inc $(CSRC)/gadapt_narrow_fwd.inc $(CSRC)/gadapt_narrow_node.inc
$(OBJDIR)/gadapt_tu_bwd_target.o: $(CSRC)/gadapt_bwd_target.inc $(CSRC)/gadapt_narrow_bwd.inc $(CSRC)/gadapt_narrow_bwd_block.inc
$(OBJDIR)/gadapt_tu_bwd_source.o: $(CSRC)/gadapt_bwd_source.inc
$(OBJDIR)/gadapt_tu_smallmesh.o: $(CSRC)/gadapt_smallmesh.inc
$(OBJDIR)/gadapt_tu_sparse.o: $(CSRC)/gadapt_sparse.inc
$(OBJDIR)/gadapt_tu_gat.o: $(CSRC)/gadapt_gat.inc
$(OBJDIR)/gadapt_tu_cnn.o: $(CSRC)/gadapt_cnn.inc $(CSRC)/gadapt_cnn_plan.h

# FLAGS_<unit>="-D..." adds flags to ONE translation unit (A/B builds of a kernel family: tools/ab_units.sh)
$(OBJDIR)/%.o: $(CSRC)/%.hip $(SHARED)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(FLAGS_$*) -c -o $@ $<

$(OBJDIR)/csr_build.o: $(CSRC)/csr_build.cpp $(CSRC)/gadapt_block_plan.h $(CSRC)/gadapt_narrow_plan.h $(TAIL_PLAN) include/gadapt_hip.h
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

resources:
	python3 tools/resources.py

clean:
	rm -rf $(OBJDIR) $(LIB) $(FEM_LIB) $(MESH_LIB)

.PHONY: all resources clean
