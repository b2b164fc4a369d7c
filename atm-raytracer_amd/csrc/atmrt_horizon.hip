// atmrt_horizon.hip — the horizon kernels (atmrt_horizon.h) on gfx950.  A translation unit of its own beside the frame pipeline, like
// the sight lines and the viewshed: the scan streams the viewshed's path table against the azimuths' profiles, the later rounds are
// one dependent chain per lane.  Built with the flags of the calling units (Makefile, CALL_EXTRA).
#define ATMRT_HORIZON_KERNELS
#include "atmrt_horizon.h"
