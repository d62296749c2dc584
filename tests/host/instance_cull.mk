# The host loops of trgl_instance_boxes / trgl_frustum_boxes (csrc/trgl_host.cpp, plain C++) under AddressSanitizer +
# UndefinedBehaviorSanitizer, as a stand-alone program (a file of its own, so that tests/host/Makefile stays as it is):
#   make -C tests/host -f instance_cull.mk instance_cull && tests/host/instance_cull_host_asan
# (tests/test_instance_cull.py builds and runs it)
CXX ?= g++
SAN := -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer
CSRC := ../../tinyrenderder_amd/csrc
instance_cull: instance_cull_host_asan
instance_cull_host_asan: instance_cull_host.cpp $(CSRC)/trgl_host.cpp $(CSRC)/scene_core.h $(CSRC)/occlusion_core.h $(CSRC)/clip_core.h ../../include/trgl.h
	$(CXX) -std=c++17 -O1 -g -ffp-contract=off $(SAN) -Wall -o $@ instance_cull_host.cpp $(CSRC)/trgl_host.cpp
clean:
	rm -f instance_cull_host_asan
.PHONY: instance_cull clean
