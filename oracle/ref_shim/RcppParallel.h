/* Stand-in for <RcppParallel.h>: selects the library's own sequential loops. */
#ifndef RCPP_PARALLEL_USE_TBB
#define RCPP_PARALLEL_USE_TBB 0
#endif
