// boost/tuple/tuple.hpp -- boost::tuple as the in-tree programs name it (projectAndStrip.cpp:20,27 `typedef boost::tuple< uint, gnSeqI,
// gnSeqI, vector< uint > > bbcol_t`).  Where a real Boost is on the include path behind this directory it is used, so this file never
// shadows it; else the standard tuple stands in under boost's name, with get, make_tuple and tie.  Nothing else of boost is here.
#ifndef MAUVE_HIP_BOOST_TUPLE_H
#define MAUVE_HIP_BOOST_TUPLE_H

#if defined(__has_include_next)
#if __has_include_next(<boost/tuple/tuple.hpp>)
#define MAUVE_HIP_REAL_BOOST_TUPLE 1
#include_next <boost/tuple/tuple.hpp>
#endif
#endif

#ifndef MAUVE_HIP_REAL_BOOST_TUPLE
#include <tuple>

namespace boost {
template <class... T> using tuple = std::tuple<T...>;
using std::get;
using std::make_tuple;
using std::tie;
}  // namespace boost
#endif
#endif
