# Top-level build: the HIP engine (libmgicp.so, gfx950) and the CPU oracle (test infra).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
PKG   := leica_point_cloud_processing_amd
LIB   := $(PKG)/libmgicp.so
SRCS  := $(PKG)/csrc/mgicp_kernels.hip $(PKG)/csrc/mgicp_engine.hip $(PKG)/csrc/mgicp_clouds.hip \
         $(PKG)/csrc/mgicp_pass.hip $(PKG)/csrc/mgicp_fod.hip $(PKG)/csrc/mgicp_comm.hip $(PKG)/csrc/mgicp_debug.hip
HDRS  := $(wildcard $(PKG)/csrc/*.hpp) include/mi355x_gicp.h include/mi355x_gicp_debug.h
# the export map: the library's dynamic symbols are the mgicp_* functions of the two headers, all else local
MAP   := $(PKG)/csrc/libmgicp.map
LDMAP := -Wl,--version-script=$(MAP)
# -ffp-contract=off: no FMA contraction, so fp32/fp64 expressions round like PCL's SSE2 Eigen
HIPFLAGS := -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -ffp-contract=off -Wall -Wno-unused-result

all: $(LIB) oracle adapter-example adapter-replay fod-replay normals-replay boundary-replay fpfh-replay corr-replay \
     harris-replay

OBJDIR := $(PKG)/csrc/build
OBJS  := $(OBJDIR)/mgicp_kernels.o $(OBJDIR)/mgicp_engine.o $(OBJDIR)/mgicp_clouds.o $(OBJDIR)/mgicp_pass.o \
         $(OBJDIR)/mgicp_fod.o $(OBJDIR)/mgicp_comm.o $(OBJDIR)/mgicp_debug.o

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

# the drop-in adapter itself (adapter/GICPAlignment.cpp + adapter/Filter_mi355x.cpp), compiled as the
# catkin package would compile it (-std=c++14, the reference's CMakeLists.txt:6) against the
# layout-exact PCL / Eigen / ROS stand-ins of tests/adapter_standins (PCL and ROS are absent here),
# linked with a replay of test/test_gicp_alignment.cpp:50-131 (test infrastructure)
STANDIN := tests/adapter_standins
REPLAY  := adapter/build/replay_test_gicp_alignment
$(REPLAY): adapter/GICPAlignment.cpp adapter/GICPAlignment.h adapter/Filter_mi355x.cpp include/mi355x_gicp.h \
           $(wildcard $(STANDIN)/*.h) $(STANDIN)/Utils_standin.cpp $(STANDIN)/replay_test_gicp_alignment.cpp $(LIB)
	mkdir -p adapter/build
	g++ -O2 -std=c++14 -Wall -Wextra -Werror -I$(STANDIN) -Iadapter -Iinclude -o $@ \
	    adapter/GICPAlignment.cpp adapter/Filter_mi355x.cpp $(STANDIN)/Utils_standin.cpp \
	    $(STANDIN)/replay_test_gicp_alignment.cpp -L$(PKG) -lmgicp -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

adapter-replay: $(REPLAY)

# adapter/FODDetector_mi355x.cpp (FODDetector::clusterPossibleFODs) compiled the same way, against the
# stand-ins above plus those of tests/adapter_standins_fod (FODDetector.h, pcl::PointIndices, the members
# the adapter leaves alone), linked with a replay of test/test_fod_detector.cpp's testFODClustering and
# testEmptyCloud (test infrastructure)
STANDIN_FOD := tests/adapter_standins_fod
FODREPLAY   := adapter/build/replay_test_fod_detector
$(FODREPLAY): adapter/FODDetector_mi355x.cpp include/mi355x_gicp.h $(wildcard $(STANDIN)/*.h) \
              $(wildcard $(STANDIN_FOD)/*.h) $(STANDIN)/Utils_standin.cpp $(STANDIN_FOD)/FODDetector_standin.cpp \
              $(STANDIN_FOD)/replay_test_fod_detector.cpp $(LIB)
	mkdir -p adapter/build
	g++ -O2 -std=c++14 -Wall -Wextra -Werror -I$(STANDIN_FOD) -I$(STANDIN) -Iadapter -Iinclude -o $@ \
	    adapter/FODDetector_mi355x.cpp $(STANDIN)/Utils_standin.cpp $(STANDIN_FOD)/FODDetector_standin.cpp \
	    $(STANDIN_FOD)/replay_test_fod_detector.cpp -L$(PKG) -lmgicp -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

fod-replay: $(FODREPLAY)

# adapter/Utils_mi355x.cpp (Utils::getNormals) compiled the same way, against the stand-ins above with the
# Utils.h of tests/adapter_standins_normals in front (getNormals and a layout-exact pcl::Normal), linked
# with a driver that runs it as InitialAlignment's constructor does (test infrastructure)
STANDIN_NRM := tests/adapter_standins_normals
NRMREPLAY   := adapter/build/replay_test_normals
$(NRMREPLAY): adapter/Utils_mi355x.cpp include/mi355x_gicp.h $(wildcard $(STANDIN)/*.h) \
              $(wildcard $(STANDIN_NRM)/*.h) $(STANDIN)/Utils_standin.cpp $(STANDIN_NRM)/replay_test_normals.cpp $(LIB)
	mkdir -p adapter/build
	g++ -O2 -std=c++14 -Wall -Wextra -Werror -I$(STANDIN_NRM) -I$(STANDIN) -Iadapter -Iinclude -o $@ \
	    adapter/Utils_mi355x.cpp $(STANDIN)/Utils_standin.cpp $(STANDIN_NRM)/replay_test_normals.cpp \
	    -L$(PKG) -lmgicp -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

normals-replay: $(NRMREPLAY)

# adapter/InitialAlignment_mi355x.cpp (InitialAlignment::obtainBoundaryKeypoints) compiled the same way: the
# InitialAlignment.h of tests/adapter_standins_boundary in front (the class with that private member), then
# the Utils.h with pcl::Normal, linked with a driver that calls it on a cloud file and a normals file
# (test infrastructure)
STANDIN_BND := tests/adapter_standins_boundary
BNDREPLAY   := adapter/build/replay_test_boundary
$(BNDREPLAY): adapter/InitialAlignment_mi355x.cpp include/mi355x_gicp.h $(wildcard $(STANDIN)/*.h) \
              $(wildcard $(STANDIN_NRM)/*.h) $(wildcard $(STANDIN_BND)/*.h) $(STANDIN)/Utils_standin.cpp \
              $(STANDIN_BND)/replay_test_boundary.cpp $(LIB)
	mkdir -p adapter/build
	g++ -O2 -std=c++14 -Wall -Wextra -Werror -I$(STANDIN_BND) -I$(STANDIN_NRM) -I$(STANDIN) -Iadapter -Iinclude -o $@ \
	    adapter/InitialAlignment_mi355x.cpp $(STANDIN)/Utils_standin.cpp $(STANDIN_BND)/replay_test_boundary.cpp \
	    -L$(PKG) -lmgicp -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

boundary-replay: $(BNDREPLAY)

# adapter/InitialAlignment_features_mi355x.cpp (InitialAlignment::obtainFeatures) compiled the same way: the
# InitialAlignment.h of tests/adapter_standins_fpfh in front (the class with that private member, its
# radius_factor_ and pcl::FPFHSignature33), linked with a driver that calls it on a cloud file, a normals
# file and a keypoint index file (test infrastructure)
STANDIN_FPFH := tests/adapter_standins_fpfh
FPFHREPLAY   := adapter/build/replay_test_fpfh
$(FPFHREPLAY): adapter/InitialAlignment_features_mi355x.cpp include/mi355x_gicp.h $(wildcard $(STANDIN)/*.h) \
               $(wildcard $(STANDIN_NRM)/*.h) $(wildcard $(STANDIN_FPFH)/*.h) $(STANDIN)/Utils_standin.cpp \
               $(STANDIN_FPFH)/replay_test_fpfh.cpp $(LIB)
	mkdir -p adapter/build
	g++ -O2 -std=c++14 -Wall -Wextra -Werror -I$(STANDIN_FPFH) -I$(STANDIN_NRM) -I$(STANDIN) -Iadapter -Iinclude -o $@ \
	    adapter/InitialAlignment_features_mi355x.cpp $(STANDIN)/Utils_standin.cpp $(STANDIN_FPFH)/replay_test_fpfh.cpp \
	    -L$(PKG) -lmgicp -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

fpfh-replay: $(FPFHREPLAY)

# adapter/InitialAlignment_correspondences_mi355x.cpp (InitialAlignment::obtainCorrespondences) compiled the
# same way: the InitialAlignment.h of tests/adapter_standins_corr in front (the class with that private
# member, its feature clouds and a pcl::Correspondence with PCL's virtual destructor), linked with a driver
# that calls it on two feature files (test infrastructure)
STANDIN_CORR := tests/adapter_standins_corr
CORRREPLAY   := adapter/build/replay_test_correspondences
$(CORRREPLAY): adapter/InitialAlignment_correspondences_mi355x.cpp include/mi355x_gicp.h $(wildcard $(STANDIN)/*.h) \
               $(wildcard $(STANDIN_NRM)/*.h) $(wildcard $(STANDIN_CORR)/*.h) $(STANDIN)/Utils_standin.cpp \
               $(STANDIN_CORR)/replay_test_correspondences.cpp $(LIB)
	mkdir -p adapter/build
	g++ -O2 -std=c++14 -Wall -Wextra -Werror -I$(STANDIN_CORR) -I$(STANDIN_NRM) -I$(STANDIN) -Iadapter -Iinclude -o $@ \
	    adapter/InitialAlignment_correspondences_mi355x.cpp $(STANDIN)/Utils_standin.cpp \
	    $(STANDIN_CORR)/replay_test_correspondences.cpp -L$(PKG) -lmgicp -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

corr-replay: $(CORRREPLAY)

# adapter/InitialAlignment_harris_mi355x.cpp (InitialAlignment::obtainHarrisKeypoints) compiled the same way:
# the InitialAlignment.h and Filter.h of tests/adapter_standins_harris in front (the class with that private
# member and its radius_factor_; Filter::extractIndices, which the member ends in), linked with a driver that
# calls it on a cloud file and a normals file (test infrastructure)
STANDIN_HAR := tests/adapter_standins_harris
HARREPLAY   := adapter/build/replay_test_harris
$(HARREPLAY): adapter/InitialAlignment_harris_mi355x.cpp include/mi355x_gicp.h $(wildcard $(STANDIN)/*.h) \
              $(wildcard $(STANDIN_NRM)/*.h) $(wildcard $(STANDIN_HAR)/*.h) $(STANDIN)/Utils_standin.cpp \
              $(STANDIN_HAR)/replay_test_harris.cpp $(LIB)
	mkdir -p adapter/build
	g++ -O2 -std=c++14 -Wall -Wextra -Werror -I$(STANDIN_HAR) -I$(STANDIN_NRM) -I$(STANDIN) -Iadapter -Iinclude -o $@ \
	    adapter/InitialAlignment_harris_mi355x.cpp $(STANDIN)/Utils_standin.cpp $(STANDIN_HAR)/replay_test_harris.cpp \
	    -L$(PKG) -lmgicp -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

harris-replay: $(HARREPLAY)

oracle:
	$(MAKE) -C oracle

clean:
	rm -f $(LIB) $(PKG)/libmgicp_*.so $(OBJS)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean adapter-example adapter-replay fod-replay normals-replay boundary-replay fpfh-replay corr-replay harris-replay variant
