/* Test-only: detmath.h's exp and sincos for tests/sky_light_model.py, one value per call. */
#include "../../atm-raytracer_amd/csrc/detmath.h"
double sl_exp(double x) { return dm_exp(x); }
void sl_sincos(double x, double* s, double* c) { dm_sincos(x, s, c); }
