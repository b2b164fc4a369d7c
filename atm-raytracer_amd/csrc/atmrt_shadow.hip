// atmrt_shadow.hip — the cast-shadow kernels (atmrt_shadow.h) on gfx950.  A translation unit of its own: the march is one long
// dependent chain per lane, like the sight lines' solve, and shares nothing with the frame's kernels but the device functions of
// atmrt_core.h / atmrt_device.h.  Built with the flags of the calling units and of the units under register pressure (Makefile:
// CALL_EXTRA, MARCH_EXTRA, MARCH_RA).
#define ATMRT_SHADOW_KERNELS
#include "atmrt_shadow.h"
