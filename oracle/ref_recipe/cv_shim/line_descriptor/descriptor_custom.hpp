#include "pli_cv_shim.hpp"
