// atmrt_viewshed.hip — the viewshed kernels (atmrt_viewshed.h) on gfx950.  A translation unit of its own beside the frame pipeline,
// like the sight lines: the path table is one dependent chain per lane, the scan streams that table against the azimuths' profiles.
// The viewshed map's scatter (atmrt_viewshed_map.h) consumes the scan's planes and is compiled here too.
// Built with the flags of the calling units (Makefile, CALL_EXTRA).
#define ATMRT_VIEWSHED_KERNELS
#include "atmrt_viewshed.h"
#include "atmrt_viewshed_map.h"
