// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-in for <boost/serialization/map.hpp>, written for this project: nothing of it is used.
#ifndef PLI_MATCH_SHIM_BOOST_SERIALIZATION_MAP_HPP
#define PLI_MATCH_SHIM_BOOST_SERIALIZATION_MAP_HPP
#include <map>
#endif
