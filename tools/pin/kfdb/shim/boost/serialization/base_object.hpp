// PIN — DEV-TIME TEST INFRASTRUCTURE ONLY.
// Stand-in for <boost/serialization/base_object.hpp>, written for this project: nothing of it is used (KeyFrameDatabase::serialize is a
// template that the pin never instantiates).
#ifndef PLI_PIN_KFDB_BOOST_BASE_OBJECT_HPP
#define PLI_PIN_KFDB_BOOST_BASE_OBJECT_HPP
#endif
