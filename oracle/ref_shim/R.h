/* Stand-in for R's <R.h>: declares the few names of R's C API that the HIBAG
 * library sources use, so that oracle.build_ref() can compile them without R.
 * Test infrastructure only.  unif_rand() is defined by oracle/ref_driver.cpp. */
#ifndef HIBAG_REF_SHIM_R_H
#define HIBAG_REF_SHIM_R_H

#include <cfloat>
#include <climits>
#include <cmath>
#include <stdexcept>

#define NA_INTEGER INT_MIN
#define R_FINITE(x) std::isfinite(x)

typedef enum { FALSE = 0, TRUE = 1 } Rboolean;

extern "C" double unif_rand(void);

static inline void Rprintf(const char *, ...) {}
static inline void R_CheckUserInterrupt(void) {}
static inline Rboolean R_ToplevelExec(void (*fun)(void *), void *data) { fun(data); return TRUE; }
[[noreturn]] static inline void Rf_error(const char *msg, ...) { throw std::runtime_error(msg); }

#endif
