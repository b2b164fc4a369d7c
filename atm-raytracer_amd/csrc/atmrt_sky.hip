// atmrt_sky.hip — the sky-ray kernels (atmrt_sky.h) on gfx950.  A translation unit of its own: the march is one long dependent
// RK4 chain per lane with nothing but the stepper alive across the loop, and shares nothing with the frame's kernels but the device
// functions of atmrt_core.h / atmrt_device.h.  Built with the flags of the march units (Makefile: CALL_EXTRA, MARCH_EXTRA, MARCH_RA),
// under which the march fits five wavefronts per SIMD without scratch (profiles/sky_resources.txt).
#define ATMRT_SKY_KERNELS
#include "atmrt_sky.h"
