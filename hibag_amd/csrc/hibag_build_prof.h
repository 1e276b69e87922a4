// hibag_build_prof.h -- the time accounts of the batched evaluation (hibag_build.hip), read by the driver's
// HIBAG_TRAIN_PROFILE report (hibag_train.hip)
#ifndef HIBAG_BUILD_PROF_H_
#define HIBAG_BUILD_PROF_H_

// where the calling thread's batched evaluations spent their time (seconds, summed until the reader zeroes them): the
// launch's host packing and, of it, the writing of the staging area and the (re)allocation of the slot; copies + kernels;
// collect's read-back and its host reductions
enum { HIBAG_BATCH_PROF_PACK = 0, HIBAG_BATCH_PROF_DEVICE, HIBAG_BATCH_PROF_READBACK, HIBAG_BATCH_PROF_REDUCE,
	HIBAG_BATCH_PROF_STAGING, HIBAG_BATCH_PROF_ALLOC, HIBAG_BATCH_PROF_N };
extern thread_local double g_batch_prof[HIBAG_BATCH_PROF_N];

#endif
