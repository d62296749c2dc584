# The host loops of the shadow post-pass (trgl_image.h) over the cases of tests/shadow_cases.py, under AddressSanitizer +
# UndefinedBehaviorSanitizer, as a stand-alone program (a file of its own, so that tests/host/Makefile stays as it is):
#   make -C tests/host -f shadow.mk shadow && tests/host/shadow_host_asan <cases file> <output file>
# (tests/test_shadow.py writes the cases, runs the program and checks its output)
CXX ?= g++
SAN := -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer
shadow: shadow_host_asan
shadow_host_asan: shadow_host.cpp ../../tinyrenderder_amd/shim/trgl_image.h
	$(CXX) -std=c++17 -O1 -g -ffp-contract=off $(SAN) -Wall -o $@ shadow_host.cpp
clean:
	rm -f shadow_host_asan
.PHONY: shadow clean
