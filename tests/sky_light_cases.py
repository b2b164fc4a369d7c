"""The frames, lists and shade inputs of the sky-light tests, in one place: tests/test_gpu_sky_light.py runs them on the GPU against
tests/sky_light_model.py, tests/test_sky_light_abi.py runs the host functions over them, and tests/test_sky_light_model.py asserts
without a GPU that every one of them holds what its case is about.  The frames and lists are tests/sky_cases.py's: 48 x 24 pixels,
lists of 0, 1, 63, 64, 65 and 257 entries, a sky step of 1000 m to a top of 100 km, m = 1500, and the short list with m = 100.  Test
infrastructure only."""
import numpy as np

import sky_cases as sc
from sky_cases import (FLOOR, FRAMES, H, H0, LIFTED_H0, LIFTED_SUN, LIST_H0, LIST_LENGTHS, M, SHORT_M, STEP, TOP, US76_SPHERE, W,  # noqa: F401
                       lifted_frame, list_elevations, list_elevations_short)

REF_ALT = 0.0  # air mass 1 is the zenith from sea level

# the same body 30 degrees up, where X is about 1.8: what the lifted sun is dimmer than
HIGH_SUN = (90.0, 30.0, LIFTED_SUN[2], LIFTED_SUN[3])

# The grid of shade inputs: one sun at (100, 3) and a wide body that holds it (the sun comes first and wins); directions at the
# sun's centre, at mu = 0.5, on the limb from inside and from outside (the radius -+ 1e-9 degrees), just outside, far outside but
# inside the wide body, and outside both; air masses from 0.7 (an observer above the reference altitude) to 40 (the horizon).
SUN = (100.0, 3.0, 0.2666, (255, 236, 170))
WIDE = (100.0, 3.0, 5.0, (200, 200, 220))
SHADE_BODIES = ([], [SUN], [SUN, WIDE], [WIDE, SUN])
SHADE_DIRECTIONS = [(100.0, 3.0), (100.0, 3.0 + 0.2666 * 0.8660254037844386), (100.0, 3.0 + 0.2666 - 1e-9), (100.0, 3.0 + 0.2666 + 1e-9),
                    (100.0, 3.0 - 0.2666 + 1e-9), (100.0, 3.0 - 0.2666 - 1e-9), (100.0 + 0.2666 / np.cos(np.radians(3.0)) - 1e-9, 3.0),
                    (100.0, 3.3), (100.0, 6.0), (104.9, 3.0), (100.0, 8.1), (250.0, 40.0), (100.13, 2.91), (99.9, 3.2)]
AIR_MASSES = (0.7, 1.0, 1.8, 5.6, 12.0, 26.3, 38.2, 40.0)
# shade parameters beside the defaults: a saturating airlight (exposure 40), no limb darkening and full limb darkening, no
# extinction, a grey airlight that never saturates
SHADE_PARAMS = (dict(),
                dict(exposure=40.0),
                dict(limb=(0.0, 0.0, 0.0)),
                dict(limb=(1.0, 1.0, 1.0), tau=(0.0, 0.5, 3.0)),
                dict(airlight=(120, 130, 140), exposure=1.0))
