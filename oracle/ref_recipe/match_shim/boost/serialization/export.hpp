// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-in for <boost/serialization/export.hpp>, written for this project: Pinhole.cpp includes it and uses nothing of it.
