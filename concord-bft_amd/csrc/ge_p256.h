// P-256 points (y^2 = x^3 - 3 x + b over GF(p)) in Jacobian coordinates (x = X / Z^2,
// y = Y / Z^3, Z = 0 is the point at infinity) for ECDSA verification.  An attacker picks u1, u2
// and Q, so no formula here assumes "generic" inputs: every addition tests for equal and opposite
// operands and for infinity and takes the doubling / infinity branch (variable time; all values
// are public).  The group has prime order, so no point has y = 0 and a doubling never leaves the
// curve's affine part except from infinity (Z3 = 2 Y Z = 0 keeps infinity at infinity).
#pragma once
#include "fe_p256.h"

struct P2Aff {  // affine point (never infinity)
  P2Fe x, y;
};
struct P2Jac {
  P2Fe x, y, z;
};

#define P2_B_LIMBS                                                                                  \
  { 0x27D2604Bu, 0x3BCE3C3Eu, 0xCC53B0F6u, 0x651D06B0u, 0x769886BCu, 0xB3EBBD55u, 0xAA3A93E7u, 0x5AC635D8u }

K1_HD void p2_ge_set_inf(P2Jac& r) {
  p2_fe_one(r.x);
  p2_fe_one(r.y);
  p2_fe_zero(r.z);
}
K1_HD bool p2_ge_is_inf(const P2Jac& p) { return p2_fe_is_zero(p.z); }
K1_HD void p2_ge_from_aff(P2Jac& r, const P2Aff& a) {
  r.x = a.x;
  r.y = a.y;
  p2_fe_one(r.z);
}
// y^2 == x^3 - 3 x + b = x (x^2 - 3) + b
K1_HD bool p2_ge_on_curve(const P2Aff& a) {
  const uint32_t B[8] = P2_B_LIMBS;
  P2Fe l, r, t;
  p2_fe_sqr(l, a.y);
  p2_fe_sqr(r, a.x);
  p2_fe_zero(t);
  t.v[0] = 3;
  p2_fe_sub(r, r, t);
  p2_fe_mul(r, r, a.x);
#pragma unroll
  for (int i = 0; i < 8; i++) t.v[i] = B[i];
  p2_fe_add(r, r, t);
  return p2_fe_eq(l, r);
}

// r = 2 p (a = -3: 4 M + 4 S).  Infinity stays infinity.
K1_HD void p2_ge_dbl(P2Jac& r, const P2Jac& p) {
  P2Fe delta, gamma, beta, alpha, t, u;
  p2_fe_sqr(delta, p.z);          // delta = Z^2
  p2_fe_sqr(gamma, p.y);          // gamma = Y^2
  p2_fe_mul(beta, p.x, gamma);    // beta = X Y^2
  p2_fe_sub(t, p.x, delta);       // M = alpha = 3 (X - Z^2) (X + Z^2)
  p2_fe_add(u, p.x, delta);
  p2_fe_mul(t, t, u);
  p2_fe_dbl(alpha, t);
  p2_fe_add(alpha, alpha, t);
  p2_fe_mul(t, p.y, p.z);         // Z3 = 2 Y Z (before X, Y change: r may be p)
  p2_fe_dbl(r.z, t);
  p2_fe_dbl(beta, beta);          // 4 beta
  p2_fe_dbl(beta, beta);
  p2_fe_sqr(t, alpha);            // X3 = alpha^2 - 8 beta
  p2_fe_dbl(u, beta);
  p2_fe_sub(r.x, t, u);
  p2_fe_sub(t, beta, r.x);        // Y3 = alpha (4 beta - X3) - 8 gamma^2
  p2_fe_mul(t, alpha, t);
  p2_fe_sqr(gamma, gamma);
  p2_fe_dbl(gamma, gamma);
  p2_fe_dbl(gamma, gamma);
  p2_fe_dbl(gamma, gamma);
  p2_fe_sub(r.y, t, gamma);
}

// r = p + q, q affine (8 M + 3 S); p = infinity, p = q and p = -q handled
K1_HD void p2_ge_madd(P2Jac& r, const P2Jac& p, const P2Aff& q) {
  if (p2_ge_is_inf(p)) {
    p2_ge_from_aff(r, q);
    return;
  }
  P2Fe zz, u2, s2, h, rr, hh, hhh, v, t;
  p2_fe_sqr(zz, p.z);
  p2_fe_mul(u2, q.x, zz);
  p2_fe_mul(s2, q.y, p.z);
  p2_fe_mul(s2, s2, zz);
  p2_fe_sub(h, u2, p.x);
  p2_fe_sub(rr, s2, p.y);
  if (p2_fe_is_zero(h)) {
    if (p2_fe_is_zero(rr)) {
      p2_ge_dbl(r, p);
    } else {
      p2_ge_set_inf(r);
    }
    return;
  }
  p2_fe_sqr(hh, h);
  p2_fe_mul(hhh, hh, h);
  p2_fe_mul(v, p.x, hh);
  p2_fe_mul(r.z, p.z, h);
  p2_fe_sqr(t, rr);          // X3 = R^2 - H^3 - 2 V
  p2_fe_sub(t, t, hhh);
  p2_fe_sub(t, t, v);
  p2_fe_sub(t, t, v);
  p2_fe_mul(hhh, hhh, p.y);  // Y1 H^3 (before r.y is written: r may be p)
  r.x = t;
  p2_fe_sub(v, v, r.x);      // Y3 = R (V - X3) - Y1 H^3
  p2_fe_mul(v, v, rr);
  p2_fe_sub(r.y, v, hhh);
}

// r = p + q, both Jacobian (12 M + 4 S); either at infinity, p = q and p = -q handled
K1_HD void p2_ge_add(P2Jac& r, const P2Jac& p, const P2Jac& q) {
  if (p2_ge_is_inf(p)) {
    r = q;
    return;
  }
  if (p2_ge_is_inf(q)) {
    r = p;
    return;
  }
  P2Fe z1z1, z2z2, u1, u2, s1, s2, h, rr, hh, hhh, v, t;
  p2_fe_sqr(z1z1, p.z);
  p2_fe_sqr(z2z2, q.z);
  p2_fe_mul(u1, p.x, z2z2);
  p2_fe_mul(u2, q.x, z1z1);
  p2_fe_mul(s1, p.y, q.z);
  p2_fe_mul(s1, s1, z2z2);
  p2_fe_mul(s2, q.y, p.z);
  p2_fe_mul(s2, s2, z1z1);
  p2_fe_sub(h, u2, u1);
  p2_fe_sub(rr, s2, s1);
  if (p2_fe_is_zero(h)) {
    if (p2_fe_is_zero(rr)) {
      p2_ge_dbl(r, p);
    } else {
      p2_ge_set_inf(r);
    }
    return;
  }
  p2_fe_sqr(hh, h);
  p2_fe_mul(hhh, hh, h);
  p2_fe_mul(v, u1, hh);
  p2_fe_mul(t, p.z, q.z);
  p2_fe_mul(r.z, t, h);
  p2_fe_sqr(t, rr);
  p2_fe_sub(t, t, hhh);
  p2_fe_sub(t, t, v);
  p2_fe_sub(t, t, v);
  r.x = t;
  p2_fe_sub(v, v, r.x);
  p2_fe_mul(v, v, rr);
  p2_fe_mul(hhh, hhh, s1);
  p2_fe_sub(r.y, v, hhh);
}

// affine form of a point that is not at infinity (one variable-time inversion)
K1_HD void p2_ge_to_aff(P2Aff& r, const P2Jac& p) {
  P2Fe zi, zi2;
  p2_fe_inv_var(zi, p.z);
  p2_fe_sqr(zi2, zi);
  p2_fe_mul(r.x, p.x, zi2);
  p2_fe_mul(zi2, zi2, zi);
  p2_fe_mul(r.y, p.y, zi2);
}
