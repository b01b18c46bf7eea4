// secp256k1 points (y^2 = x^3 + 7 over GF(p)) in Jacobian coordinates (x = X / Z^2, y = Y / Z^3,
// Z = 0 is the point at infinity) for ECDSA verification.  An attacker picks u1, u2 and Q, so no
// formula here assumes "generic" inputs: every addition tests for equal and opposite operands and
// for infinity and takes the doubling / infinity branch (variable time; all values are public).
// The group has prime order, so no point has y = 0 and a doubling never leaves the curve's affine
// part except from infinity (Z3 = 2 Y Z = 0 keeps infinity at infinity).
#pragma once
#include "fe_secp256k1.h"

struct K1Aff {  // affine point (never infinity)
  K1Fe x, y;
};
struct K1Jac {
  K1Fe x, y, z;
};

K1_HD void ge_set_inf(K1Jac& r) {
  fe_one(r.x);
  fe_one(r.y);
  fe_zero(r.z);
}
K1_HD bool ge_is_inf(const K1Jac& p) { return fe_is_zero(p.z); }
K1_HD void ge_from_aff(K1Jac& r, const K1Aff& a) {
  r.x = a.x;
  r.y = a.y;
  fe_one(r.z);
}
// y^2 == x^3 + 7
K1_HD bool ge_on_curve(const K1Aff& a) {
  K1Fe l, r, seven;
  fe_sqr(l, a.y);
  fe_sqr(r, a.x);
  fe_mul(r, r, a.x);
  fe_zero(seven);
  seven.v[0] = 7;
  fe_add(r, r, seven);
  return fe_eq(l, r);
}

// r = 2 p (a = 0: 3 M + 4 S).  Infinity stays infinity.
K1_HD void ge_dbl(K1Jac& r, const K1Jac& p) {
  K1Fe a, b, c, d, e, f, t;
  fe_sqr(a, p.x);      // A = X^2
  fe_sqr(b, p.y);      // B = Y^2
  fe_sqr(c, b);        // C = B^2
  fe_add(t, p.x, b);   // D = 2 ((X + B)^2 - A - C)
  fe_sqr(t, t);
  fe_sub(t, t, a);
  fe_sub(t, t, c);
  fe_dbl(d, t);
  fe_dbl(e, a);        // E = 3 A
  fe_add(e, e, a);
  fe_sqr(f, e);        // F = E^2
  fe_mul(t, p.y, p.z); // Z3 = 2 Y Z (before X, Y change: r may be p)
  fe_dbl(r.z, t);
  fe_dbl(t, d);        // X3 = F - 2 D
  fe_sub(r.x, f, t);
  fe_sub(t, d, r.x);   // Y3 = E (D - X3) - 8 C
  fe_mul(t, e, t);
  fe_dbl(c, c);
  fe_dbl(c, c);
  fe_dbl(c, c);
  fe_sub(r.y, t, c);
}

// r = p + q, q affine (8 M + 3 S); p = infinity, p = q and p = -q handled
K1_HD void ge_madd(K1Jac& r, const K1Jac& p, const K1Aff& q) {
  if (ge_is_inf(p)) {
    ge_from_aff(r, q);
    return;
  }
  K1Fe zz, u2, s2, h, rr, hh, hhh, v, t;
  fe_sqr(zz, p.z);
  fe_mul(u2, q.x, zz);
  fe_mul(s2, q.y, p.z);
  fe_mul(s2, s2, zz);
  fe_sub(h, u2, p.x);
  fe_sub(rr, s2, p.y);
  if (fe_is_zero(h)) {
    if (fe_is_zero(rr)) {
      ge_dbl(r, p);
    } else {
      ge_set_inf(r);
    }
    return;
  }
  fe_sqr(hh, h);
  fe_mul(hhh, hh, h);
  fe_mul(v, p.x, hh);
  fe_mul(r.z, p.z, h);
  fe_sqr(t, rr);       // X3 = R^2 - H^3 - 2 V
  fe_sub(t, t, hhh);
  fe_sub(t, t, v);
  fe_sub(t, t, v);
  fe_mul(hhh, hhh, p.y);  // Y1 H^3 (before r.y is written: r may be p)
  r.x = t;
  fe_sub(v, v, r.x);   // Y3 = R (V - X3) - Y1 H^3
  fe_mul(v, v, rr);
  fe_sub(r.y, v, hhh);
}

// r = p + q, both Jacobian (12 M + 4 S); either at infinity, p = q and p = -q handled
K1_HD void ge_add(K1Jac& r, const K1Jac& p, const K1Jac& q) {
  if (ge_is_inf(p)) {
    r = q;
    return;
  }
  if (ge_is_inf(q)) {
    r = p;
    return;
  }
  K1Fe z1z1, z2z2, u1, u2, s1, s2, h, rr, hh, hhh, v, t;
  fe_sqr(z1z1, p.z);
  fe_sqr(z2z2, q.z);
  fe_mul(u1, p.x, z2z2);
  fe_mul(u2, q.x, z1z1);
  fe_mul(s1, p.y, q.z);
  fe_mul(s1, s1, z2z2);
  fe_mul(s2, q.y, p.z);
  fe_mul(s2, s2, z1z1);
  fe_sub(h, u2, u1);
  fe_sub(rr, s2, s1);
  if (fe_is_zero(h)) {
    if (fe_is_zero(rr)) {
      ge_dbl(r, p);
    } else {
      ge_set_inf(r);
    }
    return;
  }
  fe_sqr(hh, h);
  fe_mul(hhh, hh, h);
  fe_mul(v, u1, hh);
  fe_mul(t, p.z, q.z);
  fe_mul(r.z, t, h);
  fe_sqr(t, rr);
  fe_sub(t, t, hhh);
  fe_sub(t, t, v);
  fe_sub(t, t, v);
  r.x = t;
  fe_sub(v, v, r.x);
  fe_mul(v, v, rr);
  fe_mul(hhh, hhh, s1);
  fe_sub(r.y, v, hhh);
}

// affine form of a point that is not at infinity (one variable-time inversion)
K1_HD void ge_to_aff(K1Aff& r, const K1Jac& p) {
  K1Fe zi, zi2;
  fe_inv_var(zi, p.z);
  fe_sqr(zi2, zi);
  fe_mul(r.x, p.x, zi2);
  fe_mul(zi2, zi2, zi);
  fe_mul(r.y, p.y, zi2);
}
