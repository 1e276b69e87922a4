/* Stand-in for R's <Rmath.h>: everything the HIBAG library needs is in the stand-in R.h. */
#include "R.h"
