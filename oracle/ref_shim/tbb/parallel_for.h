/* Stand-in for <tbb/parallel_for.h>: unused, RCPP_PARALLEL_USE_TBB is 0 (see RcppParallel.h). */
