// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-in for <boost/serialization/serialization.hpp>, written for this project: the two names
// DBoW2's BowVector.h and FeatureVector.h mention in their (never instantiated) serialize().
#ifndef PLI_MATCH_SHIM_BOOST_SERIALIZATION_HPP
#define PLI_MATCH_SHIM_BOOST_SERIALIZATION_HPP
namespace boost {
namespace serialization {
class access {};
template <class Base, class Derived> Base& base_object(Derived& d) { return static_cast<Base&>(d); }
}  // namespace serialization
}  // namespace boost
#endif
