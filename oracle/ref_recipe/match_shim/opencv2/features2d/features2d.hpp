// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-in for <opencv2/features2d/features2d.hpp>, written for this project: everything is in pli_match_shim.hpp.
#include "pli_match_shim.hpp"
