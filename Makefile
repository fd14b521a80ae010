# Top-level build: the HIP engine (libmgicp.so, gfx950) and the CPU oracle (test infra).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
PKG   := leica_point_cloud_processing_amd
LIB   := $(PKG)/libmgicp.so
SRCS  := $(PKG)/csrc/mgicp_kernels.hip $(PKG)/csrc/mgicp_engine.hip $(PKG)/csrc/mgicp_clouds.hip \
         $(PKG)/csrc/mgicp_pass.hip $(PKG)/csrc/mgicp_fod.hip $(PKG)/csrc/mgicp_features.hip $(PKG)/csrc/mgicp_comm.hip \
         $(PKG)/csrc/mgicp_debug.hip
HDRS  := $(wildcard $(PKG)/csrc/*.hpp) include/mi355x_gicp.h include/mi355x_gicp_debug.h
# the export map: the library's dynamic symbols are the mgicp_* functions of the two headers, all else local
MAP   := $(PKG)/csrc/libmgicp.map
LDMAP := -Wl,--version-script=$(MAP)
# -ffp-contract=off: no FMA contraction, so fp32/fp64 expressions round like PCL's SSE2 Eigen
HIPFLAGS := -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -ffp-contract=off -Wall -Wno-unused-result

all: $(LIB) oracle adapter-example adapter-replay fod-replay normals-replay boundary-replay fpfh-replay corr-replay \
     harris-replay ia-replay transform-replay normals-cluster-replay

OBJDIR := $(PKG)/csrc/build
OBJS  := $(OBJDIR)/mgicp_kernels.o $(OBJDIR)/mgicp_engine.o $(OBJDIR)/mgicp_clouds.o $(OBJDIR)/mgicp_pass.o \
         $(OBJDIR)/mgicp_fod.o $(OBJDIR)/mgicp_features.o $(OBJDIR)/mgicp_comm.o $(OBJDIR)/mgicp_debug.o

# one object per source (make -j compiles them side by side; an engine edit does not rebuild the kernels)
$(OBJDIR)/%.o: $(PKG)/csrc/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(LIB): $(OBJS) $(MAP)
	$(HIPCC) $(HIPFLAGS) -shared $(LDMAP) -o $@ $(OBJS) -lrccl

# diagnostic builds: make variant NAME=diag DEFS=-DMGICP_CORR_PHASES=1 -> libmgicp_diag.so (MGICP_LIB_NAME selects it)
variant: $(SRCS) $(HDRS) $(MAP)
	$(HIPCC) $(HIPFLAGS) $(DEFS) -shared $(LDMAP) -o $(PKG)/libmgicp_$(NAME).so $(SRCS) -lrccl

# plain C++ host program over the C-ABI (g++, no HIP headers): what an integrator links
adapter/cabi_example: adapter/cabi_example.cpp include/mi355x_gicp.h $(LIB)
	g++ -O2 -std=c++14 -Wall -Iinclude -o $@ adapter/cabi_example.cpp -L$(PKG) -lmgicp -Wl,-rpath,'$$ORIGIN/../$(PKG)'

adapter-example: adapter/cabi_example

# The adapter files, each compiled as the catkin package would compile it (-std=c++14, the reference's
# CMakeLists.txt:6) against layout-exact PCL / Eigen / ROS stand-ins (PCL and ROS are absent here) and
# linked with a replay driver (test infrastructure).  tests/adapter_standins holds the common stand-ins;
# a directory in front of it on the include path adds or replaces the headers of one adapter file.
#   $(call replay_rule,<target>,<binary under adapter/build>,<adapter sources>,
#          <stand-in directories, the first in front>,<stand-in sources and the driver>)
STANDIN     := tests/adapter_standins
STANDIN_FOD := tests/adapter_standins_fod
STANDIN_NRM := tests/adapter_standins_normals
STANDIN_IA  := tests/adapter_standins_ia
STANDIN_IAT := tests/adapter_standins_ia_transform
STANDIN_IAN := tests/adapter_standins_ia_normals
define replay_rule
adapter/build/$(2): $(3) $$(wildcard adapter/*.h) include/mi355x_gicp.h $$(foreach d,$(4),$$(wildcard $$(d)/*.h)) $(5) $$(LIB)
	mkdir -p adapter/build
	g++ -O2 -std=c++14 -Wall -Wextra -Werror $$(addprefix -I,$(4)) -Iadapter -Iinclude -o $$@ \
	    $(3) $(5) -L$$(PKG) -lmgicp -Wl,-rpath,'$$$$ORIGIN/../../$$(PKG)'

$(1): adapter/build/$(2)
endef

# adapter/GICPAlignment.cpp + adapter/Filter_mi355x.cpp: a replay of test/test_gicp_alignment.cpp:50-131
$(eval $(call replay_rule,adapter-replay,replay_test_gicp_alignment,adapter/GICPAlignment.cpp adapter/Filter_mi355x.cpp,\
  $(STANDIN),$(STANDIN)/Utils_standin.cpp $(STANDIN)/replay_test_gicp_alignment.cpp))
# adapter/FODDetector_mi355x.cpp (FODDetector::clusterPossibleFODs): FODDetector.h, pcl::PointIndices and the
# members the adapter leaves alone in front; a replay of test/test_fod_detector.cpp's testFODClustering and
# testEmptyCloud
$(eval $(call replay_rule,fod-replay,replay_test_fod_detector,adapter/FODDetector_mi355x.cpp,$(STANDIN_FOD) $(STANDIN),\
  $(STANDIN)/Utils_standin.cpp $(STANDIN_FOD)/FODDetector_standin.cpp $(STANDIN_FOD)/replay_test_fod_detector.cpp))
# adapter/Utils_mi355x.cpp (Utils::getNormals): the Utils.h with getNormals and a layout-exact pcl::Normal in
# front; a driver that runs it as InitialAlignment's constructor does
$(eval $(call replay_rule,normals-replay,replay_test_normals,adapter/Utils_mi355x.cpp,$(STANDIN_NRM) $(STANDIN),\
  $(STANDIN)/Utils_standin.cpp $(STANDIN_NRM)/replay_test_normals.cpp))
# adapter/InitialAlignment_mi355x.cpp (obtainBoundaryKeypoints, obtainHarrisKeypoints, obtainFeatures,
# obtainCorrespondences): the InitialAlignment.h and Filter.h of tests/adapter_standins_ia in front, then the
# Utils.h with pcl::Normal; one driver per member, each on files of its inputs, and one that runs the four
# members in one process
IA_REPLAYS := boundary-replay:replay_test_boundary fpfh-replay:replay_test_fpfh corr-replay:replay_test_correspondences \
              harris-replay:replay_test_harris ia-replay:replay_test_initial_alignment
$(foreach r,$(IA_REPLAYS),$(eval $(call replay_rule,$(word 1,$(subst :, ,$(r))),$(word 2,$(subst :, ,$(r))),\
  adapter/InitialAlignment_mi355x.cpp,$(STANDIN_IA) $(STANDIN_NRM) $(STANDIN),\
  $(STANDIN)/Utils_standin.cpp $(STANDIN_IA)/Filter_standin.cpp $(STANDIN_IA)/$(word 2,$(subst :, ,$(r))).cpp)))
# adapter/InitialAlignment_transform_mi355x.cpp (rejectCorrespondences, rejectOneToOneCorrespondences,
# estimateTransform): the InitialAlignment.h with the keypoint clouds, the correspondences and rigid_tf_ in
# front; one driver that runs the three members in runKeypointsBasedAlgorithm's order on files of their inputs
$(eval $(call replay_rule,transform-replay,replay_test_transform,adapter/InitialAlignment_transform_mi355x.cpp,\
  $(STANDIN_IAT) $(STANDIN),$(STANDIN)/Utils_standin.cpp $(STANDIN_IAT)/replay_test_transform.cpp))
# adapter/InitialAlignment_normals_mi355x.cpp (obtainNormalsCluster, obtainDominantNormals): the
# InitialAlignment.h with pcl::PointIndices in front, then the Utils.h with pcl::Normal; one driver that runs the
# two members in runNormalsBasedAlgorithm's order on files of their inputs
$(eval $(call replay_rule,normals-cluster-replay,replay_test_normals_cluster,adapter/InitialAlignment_normals_mi355x.cpp,\
  $(STANDIN_IAN) $(STANDIN_NRM) $(STANDIN),$(STANDIN)/Utils_standin.cpp $(STANDIN_IAN)/replay_test_normals_cluster.cpp))

oracle:
	$(MAKE) -C oracle

clean:
	rm -f $(LIB) $(PKG)/libmgicp_*.so $(OBJS)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean adapter-example adapter-replay fod-replay normals-replay boundary-replay fpfh-replay corr-replay harris-replay ia-replay transform-replay normals-cluster-replay variant
