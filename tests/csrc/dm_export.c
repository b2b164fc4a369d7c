/* Test-only: exports detmath.h functions over arrays so tests/test_detmath.py can bound them against libm. */
#include "../../atm-raytracer_amd/csrc/detmath.h"
#include <stddef.h>
#define V1(name) void t_##name(const double* x, double* y, size_t n) { for (size_t i = 0; i < n; i++) y[i] = dm_##name(x[i]); }
V1(sin) V1(cos) V1(tan) V1(asin) V1(atan) V1(exp) V1(log) V1(sqrt) V1(floor)
void t_atan2(const double* a, const double* b, double* y, size_t n) { for (size_t i = 0; i < n; i++) y[i] = dm_atan2(a[i], b[i]); }
void t_pow(const double* a, const double* b, double* y, size_t n) { for (size_t i = 0; i < n; i++) y[i] = dm_pow(a[i], b[i]); }
void t_div_r_seq(const double* a, const double* b, double* y, size_t n) { for (size_t i = 0; i < n; i++) y[i] = dm_div_r_seq(a[i], b[i], 1.0 / b[i]); }
/* host counterparts of atmrt_math_probe (tests/test_gpu_detmath.py): on the host dm_div / dm_div_r / dm_sqrt_inrange ARE the IEEE operations */
void t_div(const double* a, const double* b, double* y, size_t n) { for (size_t i = 0; i < n; i++) y[i] = dm_div(a[i], b[i]); }
void t_div_r(const double* a, const double* b, double* y, size_t n) { for (size_t i = 0; i < n; i++) y[i] = dm_div_r(a[i], b[i], 1.0 / b[i]); }
V1(sqrt_inrange)
void t_sincos(const double* x, double* s, double* c, size_t n) { for (size_t i = 0; i < n; i++) dm_sincos(x[i], &s[i], &c[i]); }
void t_pow3(const double* a, const double* b, double* y0, double* y1, size_t n) {
  for (size_t i = 0; i < n; i++) {
    y0[i] = dm_pow(a[i], b[i]);
    y1[i] = dm_pow(a[i] * 0.99999981, b[i]) + dm_pow(a[i] * 1.00000019, b[i]);
  }
}
void t_div3(const double* a, const double* b, double* y0, double* y1, size_t n) {
  for (size_t i = 0; i < n; i++) {
    double q0;
    dm_div3(a[i], b[i], a[i], b[i] * 0.99999976158142090, a[i], b[i] * 1.00000047683715820, &q0, &y0[i], &y1[i]);
  }
}
void t_div3_seeded(const double* a, const double* b, double* y0, double* y1, size_t n) {
  for (size_t i = 0; i < n; i++) {
    double q0;
    dm_div3_seeded(a[i], b[i], a[i], b[i] * 0.99999976158142090, a[i], b[i] * 1.00000023841857910, 0, 0.0, &q0, &y0[i], &y1[i]);
  }
}
void t_div3_seed_z(const double* a, const double* b, double* y0, double* y1, size_t n) {
  for (size_t i = 0; i < n; i++) {
    double q1;
    dm_div3_seeded(a[i], b[i], a[i], b[i] * 0.99999976158142090, a[i], b[i] * 1.00000023841857910, 1, 2.0 - b[i], &y0[i], &q1, &y1[i]);
  }
}
void t_div_seed_n(const double* a, const double* b, double* y, size_t n) {
  for (size_t i = 0; i < n; i++) y[i] = dm_div_seeded(a[i], 1.0 + b[i], 1.0 - b[i]);
}
/* host counterparts of atmrt_math_probe3: the plain operation per point, every operand the caller's */
void t_div3x(const double* a, const double* b0, const double* b1, const double* b2, double* y0, double* y1, double* y2, size_t n) {
  for (size_t i = 0; i < n; i++) y0[i] = a[i] / b0[i], y1[i] = a[i] / b1[i], y2[i] = a[i] / b2[i];
}
void t_pow3x(const double* a, const double* b0, const double* b1, const double* b2, double* y0, double* y1, double* y2, size_t n) {
  for (size_t i = 0; i < n; i++) y0[i] = dm_pow(b0[i], a[i]), y1[i] = dm_pow(b1[i], a[i]), y2[i] = dm_pow(b2[i], a[i]);
}
void t_exp3x(const double* a, const double* b0, const double* b1, const double* b2, double* y0, double* y1, double* y2, size_t n) {
  for (size_t i = 0; i < n; i++) y0[i] = dm_exp_main(a[i] * b0[i]), y1[i] = dm_exp_main(a[i] * b1[i]), y2[i] = dm_exp_main(a[i] * b2[i]);
}
/* what a lane contributes to the wave votes of pow3_tight(b0, ., ., y = a, thr) (isothermal = 0) or exp3_tight(a b0, ., ., thr) (1):
 * log_ok: the centre argument is not on the edge of its log table interval (dm_log3_core_pow_shared); exp_ok: the centre's exponent
 * product is at least 1/2 - thr away from a half-integer of 128 / ln2 (dm_exp3_main_shared).  The test ANDs them over 64 lanes. */
void t_vote3(const double* a, const double* b0, const double* thr, int isothermal, int32_t* log_ok, int32_t* exp_ok, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const uint32_t hi = (uint32_t)(dm_bits(b0[i]) >> 32);
    log_ok[i] = isothermal || ((hi + 0x1000u) & 0x1fffu) - 1u < 0x1ffeu;
    const double e0 = isothermal ? a[i] * b0[i] : a[i] * dm_log_core_pow(b0[i]);
    const double t0 = e0 * DM_INVLN2N;
    exp_ok[i] = dm_fabs(t0 - dm_rint(t0)) <= thr[i];
  }
}
void t_pow3_shared(const double* a, const double* b, double* y0, double* y1, size_t n) {
  for (size_t i = 0; i < n; i++) {
    y0[i] = dm_pow(a[i], b[i]);
    y1[i] = dm_pow(a[i] * 0.99999976158142090, b[i]) + dm_pow(a[i] * 1.00000023841857910, b[i]);
  }
}
