/* Stand-in for R's <Rinternals.h>: everything the HIBAG library needs is in the stand-in R.h. */
#include "R.h"
