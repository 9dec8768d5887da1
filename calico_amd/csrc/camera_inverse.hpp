// camera_inverse.hpp — the inverse of project<MODEL> (device_math.hpp): pixel -> unit-norm point.
//
// unproject<MODEL>(k, u, v) is the point b with |b| = 1 and project<MODEL>(k, b) == (u, v) under THIS library's
// projection, the one a calibration was estimated with (sensors::CameraModel::UnprojectPixel, camera_models.h, is the
// interface it stands for). For six models b is the usual bearing: their projection does not depend on the point's norm.
// ExtendedUnified (quirk Q5b, next to Q5): the projection evaluated here and in the reference is d = sqrt(beta |p_xy| + z^2) -- the
// norm, not its square --, which is not scale invariant, so "the unit-norm point that projects to the pixel" is the
// definition, and the reference's closed form (the inverse of the textbook model: its header calls it "rather imprecise",
// its test allows 2e-2) is not reproduced.
//   DoubleSphere, FieldOfView, Unified   closed forms, exact inverses of project<>
//   OpenCv5, OpenCv8                      Newton in 2-D on the normalised point, at most kNewtonCapOpenCv steps
//   KannalaBrandt, ExtendedUnified        Newton in 1-D on the polar angle, at most kNewtonCapAngle steps
// Stop rule of the iterations: |error| < 1e-14 in normalised units (pixel error / f), the reference's. A lane that has
// converged is frozen; on the device the wave leaves the loop when every lane has converged or the cap is reached.
// Returns false -- the caller writes zeros -- when Newton did not reach the stop rule, a closed form's radicand is negative,
// the result is not finite, project<> rejects the resulting point, or its pixel is not the one asked for (1e-9 normalised).
// Compiles for the host as well (one "lane"): the same code can be checked without a device.
#pragma once
#include "device_math.hpp"

namespace cal {

constexpr double kUnprojectTol = 1e-14;
// project<>(b) against the pixel, normalised units: five orders above the stop rule (conditioning at the image's edge, the
// forward model's own jump between FieldOfView's branches, 2.5e-11), far below anything a wrong root or branch leaves
constexpr double kReprojectTol = 1e-9;
constexpr int kNewtonCapOpenCv = 30;
constexpr int kNewtonCapAngle = 100;

#if defined(__HIP_DEVICE_COMPILE__)
DEV bool all_lanes(bool v) { return __all(v) != 0; }      // over the lanes that are active at the call
#else
DEV bool all_lanes(bool v) { return v; }
#endif
DEV double dabs(double a) { return __builtin_fabs(a); }
DEV bool finite3(V3 a) { return __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z); }
DEV V3 unit(V3 a) { return (1.0 / sqrt(dot(a, a))) * a; }

// `live` = false: a lane without a pixel (the tail of the last wave) -- it counts as converged from the start.
template <int MODEL>
DEV bool unproject(const double* __restrict__ k, double u, double v, bool live, V3* out) {
  const double inv_f = 1.0 / k[0];
  const double mx = (u - k[1]) * inv_f, my = (v - k[2]) * inv_f;
  V3 b = mk(0.0, 0.0, 1.0);
  bool ok = live;
  if constexpr (MODEL == 1 || MODEL == 2) {
    const double k1 = k[3], k2 = k[4], p1 = k[5], p2 = k[6], k3 = k[7];
    double x = mx, y = my;
    bool done = !live, conv = false;
    for (int it = 0;; ++it) {
      const double r2 = x * x + y * y;
      const double num = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
      const double nump = k1 + r2 * (2.0 * k2 + 3.0 * r2 * k3);
      double s = num, sp = nump;      // radial factor and d s / d r2
      if constexpr (MODEL == 2) {
        const double iden = 1.0 / (1.0 + r2 * (k[8] + r2 * (k[9] + r2 * k[10])));
        s = num * iden;
        sp = (nump - s * (k[8] + r2 * (2.0 * k[9] + 3.0 * r2 * k[10]))) * iden;
      }
      const double ex = mx - (x * s + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x));
      const double ey = my - (y * s + 2.0 * p2 * x * y + p1 * (r2 + 2.0 * y * y));
      if (!done && dabs(ex) + dabs(ey) < kUnprojectTol) { done = true; conv = true; }
      if (it == kNewtonCapOpenCv || all_lanes(done)) break;
      if (!done) {
        const double a = s + 2.0 * x * x * sp + 2.0 * p1 * y + 6.0 * p2 * x;
        const double c = 2.0 * x * y * sp + 2.0 * p1 * x + 2.0 * p2 * y;
        const double d = s + 2.0 * y * y * sp + 2.0 * p2 * x + 6.0 * p1 * y;
        const double idet = 1.0 / (a * d - c * c);
        x += idet * (d * ex - c * ey);
        y += idet * (a * ey - c * ex);
      }
    }
    ok = ok && conv;
    b = unit(mk(x, y, 1.0));
  } else if constexpr (MODEL == 3) {
    const double k1 = k[3], k2 = k[4], k3 = k[5], k4 = k[6];
    const double rd = sqrt(mx * mx + my * my);
    double th = rd;
    bool done = !live, conv = false;
    for (int it = 0;; ++it) {
      const double t2 = th * th;
      const double g = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - rd;
      if (!done && dabs(g) < kUnprojectTol) { done = true; conv = true; }
      if (it == kNewtonCapAngle || all_lanes(done)) break;
      if (!done) th -= g / (1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * 9.0 * k4))));
    }
    ok = ok && conv;
    double st, ct;
    dsincos(th, &st, &ct);
    const double q = rd > 0.0 ? st / rd : 0.0;
    b = mk(q * mx, q * my, ct);
  } else if constexpr (MODEL == 4) {
    // Usenko, Demmel, Cremers, "The Double Sphere Camera Model" (3DV 2018), eq. (47)-(50)
    const double xi = k[3], al = k[4];
    const double r2 = mx * mx + my * my;
    const double rad1 = 1.0 - (2.0 * al - 1.0) * r2;
    ok = ok && rad1 >= 0.0;
    const double mz = (1.0 - al * al * r2) / (al * sqrt(fmax(rad1, 0.0)) + 1.0 - al);
    const double rad2 = mz * mz + (1.0 - xi * xi) * r2;
    ok = ok && rad2 >= 0.0;
    const double s = (mz * xi + sqrt(fmax(rad2, 0.0))) / (mz * mz + r2);
    b = unit(mk(s * mx, s * my, s * mz - xi));
  } else if constexpr (MODEL == 5) {
    // project<5>: distorted radius rd = atan(r tt) / w, tt = 2 tan(w / 2); its branches for a small w and a small r are
    // followed (at r^2 = 1e-5 the forward model itself jumps from one to the other)
    const double w = k[3];
    const double rd = sqrt(mx * mx + my * my);
    double r = rd;
    if (w * w >= 1e-5) {
      const double tt = 2.0 * tan(w * 0.5);
      const double r_small = rd * w / tt;
      if (r_small * r_small < 1e-5) r = r_small;
      else {
        double sa, ca;
        dsincos(rd * w, &sa, &ca);
        ok = ok && ca > 0.0;      // beyond a quarter turn no point in front of the camera projects there
        r = sa / (ca * tt);
      }
    }
    const double q = rd > 0.0 ? r / rd : 0.0;
    b = unit(mk(q * mx, q * my, 1.0));
  } else if constexpr (MODEL == 6) {
    // unit b = (X, Y, z): m (al + (1 - al) z) = (X, Y) and X^2 + Y^2 = 1 - z^2 give a quadratic in z, whose root with
    // al + (1 - al) z > 0 is taken
    const double al = k[3], be = 1.0 - al;
    const double r2 = mx * mx + my * my;
    const double rad = 1.0 + r2 * (be * be - al * al);
    ok = ok && rad >= 0.0;
    const double z = (sqrt(fmax(rad, 0.0)) - r2 * al * be) / (r2 * be * be + 1.0);
    const double den = al + be * z;
    b = unit(mk(mx * den, my * den, z));
  } else {
    // unit b = (sin th * m / |m|, cos th):  sin th / (al sqrt(be sin th + cos^2 th) + (1 - al) cos th) = |m|
    const double al = k[3], be = k[4];
    const double mr = sqrt(mx * mx + my * my);
    double th = atan(mr);
    bool done = !live, conv = false;
    double st, ct;
    for (int it = 0;; ++it) {
      dsincos(th, &st, &ct);
      const double d = sqrt(be * st + ct * ct);
      const double den = al * d + (1.0 - al) * ct;
      const double h = st / den - mr;
      if (!done && dabs(h) < kUnprojectTol) { done = true; conv = true; }
      if (it == kNewtonCapAngle || all_lanes(done)) break;
      if (!done) {
        const double dden = al * (0.5 * be - st) * ct / d - (1.0 - al) * st;
        const double hp = (ct * den - st * dden) / (den * den);
        th -= h / hp;
        th = th < 0.0 ? 0.0 : (th > 3.1 ? 3.1 : th);      // (sin th >= 0: the radicand stays positive)
      }
    }
    ok = ok && conv;
    dsincos(th, &st, &ct);
    const double q = mr > 0.0 ? st / mr : 0.0;
    b = mk(q * mx, q * my, ct);
  }
  ok = ok && finite3(b);
  if (ok) {      // valid means what it says: the point projects, and onto this pixel
    double pix[2];
    ok = project<MODEL, false>(k, b, pix, nullptr, nullptr) && (dabs(pix[0] - u) + dabs(pix[1] - v)) * dabs(inv_f) <= kReprojectTol;
  }
  *out = ok ? b : mk(0.0, 0.0, 0.0);
  return ok;
}

}  // namespace cal
