#include "pli_line_shim.hpp"
