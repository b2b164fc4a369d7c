// atmrt_sight.hip — the sight-line kernels (atmrt_sight.h) on gfx950.  A translation unit of its own: the solve is one long
// dependent chain per lane, like phase B of the Fast generator, and shares nothing with the frame's kernels but the device functions
// of atmrt_core.h / atmrt_device.h.  Built with the flags of the calling units (Makefile, CALL_EXTRA).
#define ATMRT_SIGHT_KERNELS
#include "atmrt_sight.h"
