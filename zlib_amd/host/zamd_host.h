/* zamd_host.h -- internal (not installed): what the files of the host library share.  Not exported from libzamd_z.so. */
#ifndef ZAMD_HOST_H
#define ZAMD_HOST_H
#include "../../include/zamd_gpu.h"

/* zamd_batch.c: the engine of the batch calls (created on first use, on the device ZAMD_DEVICE names) behind its lock -- one call at a time.
 * NULL: no engine, and the lock is not held.  Every successful zamd_batch_engine_lock() is followed by one zamd_batch_engine_unlock(). */
zgpu_engine *zamd_batch_engine_lock(void);
void zamd_batch_engine_unlock(void);

#endif
