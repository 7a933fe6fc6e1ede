// ORACLE -- TEST INFRASTRUCTURE ONLY.  Everything this name stands for is in pli_stereo_shim.hpp, which oracle/Makefile force-includes.
