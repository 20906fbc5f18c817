// Analytic per-slot derivatives of the validation loss (vtd_loss.hip), float32: the
// derivatives of the graph the reference builds (tests/loss_grad_oracle.py restates it for
// torch.autograd), w.r.t. the decoded prediction.  Products that feed an add or a subtract go
// through rounded() (vtd_box.h), as in the forward.  Two deliberate deviations from autodiff
// of the reference, DESIGN.md "Loss gradients":
//  - r_diou is differentiated as (dx^2 + dy^2) / (c + eps)^2, not through the sqrt of the
//    centre distance: the same value, finite (0 in x and y) at coincident centres where the
//    sqrt's derivative is 0/0;
//  - at a kink (tied edges, a zero class error, boxes that just touch) one of the one-sided
//    derivatives is returned, always finite.
#pragma once

#include "vtd_box.h"

namespace vtd {

// d sorted[k] / d e_i of the reference's ascending sort of one axis' four edges
// [label near, label far, prediction near, prediction far]: 1 where edge i lands at position
// k.  Ties resolve as a stable sort does (an equal edge earlier in the list sorts first).
// Returns the positions of the prediction's near and far edge.
__device__ __forceinline__ void edge_ranks(float ln, float lf, float pn, float pf, int* rn,
                                           int* rf) {
  *rn = (int)(ln <= pn) + (int)(lf <= pn) + (int)(pf < pn);
  *rf = (int)(ln <= pf) + (int)(lf <= pf) + (int)(pn <= pf);
}

// One axis (centre c, size s of both boxes): the derivatives of the intersection length
// sorted[2] - sorted[1] (only under the reference's intersect condition `cond`) and of the
// enclosing length sorted[3] - sorted[0] w.r.t. the prediction's centre and size.
struct AxisGrad {
  float inter_c, inter_s;      // d intersection length / d centre, / d size
  float encl_c, encl_s;        // d enclosing length / d centre, / d size
};
__device__ __forceinline__ AxisGrad axis_grad(float lc, float ls, float pc, float ps, bool cond) {
  const float ln = lc - ls / 2.f, lf = lc + ls / 2.f;
  const float pn = pc - ps / 2.f, pf = pc + ps / 2.f;
  int rn, rf;
  edge_ranks(ln, lf, pn, pf, &rn, &rf);
  // near edge = c - s / 2, far edge = c + s / 2
  const float in = cond ? (float)((rn == 2) - (rn == 1)) : 0.f;
  const float jf = cond ? (float)((rf == 2) - (rf == 1)) : 0.f;
  const float en = (float)((rn == 3) - (rn == 0));
  const float ef = (float)((rf == 3) - (rf == 0));
  AxisGrad g;
  g.inter_c = in + jf;
  g.inter_s = (jf - in) * 0.5f;
  g.encl_c = en + ef;
  g.encl_s = (ef - en) * 0.5f;
  return g;
}

// d ciou_calculator / d (px, py, ph, pw) for one pair of (x, y, h, w) boxes: the CIoU loss
// 1 - iou + r_diou + alpha v with the gradient through iou, r_diou, v and alpha (the
// reference has no stop_gradient), or the DIoU iou - r_diou with `get_diou`.
__device__ __forceinline__ void ciou_grad_one(const float* l, const float* p, bool get_diou,
                                              float* g) {
  const float lx = l[0], ly = l[1], lh = l[2], lw = l[3];
  const float px = p[0], py = p[1], ph = p[2], pw = p[3];
  const float ll = lx - lw / 2.f, lr = lx + lw / 2.f;
  const float pl = px - pw / 2.f, pr = px + pw / 2.f;
  const float lt = ly - lh / 2.f, lb = ly + lh / 2.f;
  const float pt = py - ph / 2.f, pb = py + ph / 2.f;
  const bool cond = (ll < pr) && (lr > pl) && (lt < pb) && (lb > pt);
  const AxisGrad ax = axis_grad(lx, lw, px, pw, cond);     // x and width
  const AxisGrad ay = axis_grad(ly, lh, py, ph, cond);     // y and height
  // iou = inter / (uni + eps), uni = pw ph + lw lh - inter, inter = ih iw (iou_one)
  const float ih = cond ? fminf(lb, pb) - fmaxf(lt, pt) : 0.f;
  const float iw = cond ? fminf(lr, pr) - fmaxf(ll, pl) : 0.f;
  const float inter = rounded(ih * iw);
  const float U = ((rounded(pw * ph) + rounded(lw * lh)) - inter) + 1e-8f;
  const float iou = inter / U;
  // d inter, then d iou = (d inter - iou d uni) / U with d uni = d (pw ph) - d inter
  const float di[4] = {ih * ax.inter_c, iw * ay.inter_c, iw * ay.inter_s, ih * ax.inter_s};
  const float da[4] = {0.f, 0.f, pw, ph};                  // d (pw ph)
  // (one reciprocal per denominator, then multiplies: a division costs ten instructions)
  const float rU = 1.f / U;
  float diou[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) diou[k] = (di[k] - rounded(iou * (da[k] - di[k]))) * rU;
  // r_diou = rho2 / C^2, C = c + eps, c = sqrt(eh^2 + ew^2) of the enclosing box
  const float dx = lx - px, dy = ly - py;
  const float rho2 = rounded(dx * dx) + rounded(dy * dy);
  const float eh = fmaxf(fmaxf(lt, lb), fmaxf(pt, pb)) - fminf(fminf(lt, lb), fminf(pt, pb));
  const float ew = fmaxf(fmaxf(ll, lr), fmaxf(pl, pr)) - fminf(fminf(ll, lr), fminf(pl, pr));
  const float c = sqrtf(rounded(eh * eh) + rounded(ew * ew));
  const float C = c + 1e-8f;
  const float rC2 = 1.f / (C * C);
  // d r = d rho2 / C^2 - 2 rho2 dc / C^3, dc = (eh d eh + ew d ew) / c (0 for a point)
  const float k3 = c > 0.f ? ((-2.f * rho2) * rC2) / (C * c) : 0.f;
  const float drho[4] = {-2.f * dx, -2.f * dy, 0.f, 0.f};
  const float de[4] = {ew * ax.encl_c, eh * ay.encl_c, eh * ay.encl_s, ew * ax.encl_s};
  float dr[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) dr[k] = rounded(drho[k] * rC2) + rounded(k3 * de[k]);
  if (get_diou) {
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = diou[k] - dr[k];
    return;
  }
  // v = (al - ap)^2 4 / pi2, ap = atan(pw / H), H = ph + eps:
  // d ap / d pw = H / (H^2 + pw^2), d ap / d ph = -pw / (H^2 + pw^2)
  constexpr float kPi = 3.14159265358979323846f;
  constexpr float kPiSq = kPi * kPi;
  const float H = ph + 1e-8f;
  const float al = atanf(lw / (lh + 1e-8f));
  const float ap = atanf(pw / H);
  const float dap = al - ap;
  const float v = ((dap * dap) * 4.f) / kPiSq;
  const float D = ((1.f - iou) + v) + 1e-8f;
  const float alpha = v / D;
  const float q = rounded(H * H) + rounded(pw * pw);
  const float s = ((-2.f * dap) * 4.f) / kPiSq;           // d v / d ap
  const float sq = q > 0.f ? s / q : 0.f;
  const float dv[4] = {0.f, 0.f, sq * -pw, sq * H};
  // alpha = v / D: d alpha = (dv (D - v) + v d iou) / D^2; loss = 1 - iou + r + alpha v
  const float DmV = (1.f - iou) + 1e-8f;
  const float rD2 = 1.f / (D * D);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float dalpha = (rounded(dv[k] * DmV) + rounded(v * diou[k])) * rD2;
    g[k] = ((dr[k] - diou[k]) + rounded(dalpha * v)) + rounded(alpha * dv[k]);
  }
}

// d (objectness term of one slot) / d p: the Keras binary cross-entropy on
// p_c = clip(p, 1e-7, 1 - 1e-7) -- the clip passes the gradient on its closed interval, as
// tf.clip_by_value and torch.clamp do -- times, in the focal form, (1 - p_t)^2 of the
// unclipped p, which is differentiated too.
__device__ __forceinline__ float objectness_grad(float y, float p, bool focal) {
  const float lo = 1e-7f, hi = 1.f - 1e-7f;
  const float pc = fminf(fmaxf(p, lo), hi);
  const float pass = (p >= lo && p <= hi) ? 1.f : 0.f;
  const float a = pc + 1e-7f, b = (1.f - pc) + 1e-7f;
  // bce = -(y log a + (1 - y) log b)
  const float dbce = pass * (rounded((1.f - y) / b) - rounded(y / a));
  if (!focal) return dbce;
  const float bce = -(rounded(y * logf(a)) + rounded((1.f - y) * logf(b)));
  const float pt = rounded(y * p) + rounded((1.f - y) * (1.f - p));
  const float f = 1.f - pt;                                // d f / d p = 1 - 2 y
  return rounded((2.f * f) * (1.f - (y + y)) * bce) + rounded((f * f) * dbce);
}

// d (coefficient |delta|)^exponent / d delta = exponent coefficient (coefficient
// |delta|)^(exponent - 1) sign(delta), sign(0) = 0; exponent >= 1 (checked on the host).
__device__ __forceinline__ float class_grad(float delta, float coefficient, float exponent) {
  const float ce = coefficient * fabsf(delta);
  const float sign = delta > 0.f ? 1.f : (delta < 0.f ? -1.f : 0.f);
  if (sign == 0.f) return 0.f;
  const float pw = exponent == 2.f ? ce : (exponent == 1.f ? 1.f : powf(ce, exponent - 1.f));
  return (exponent * coefficient) * pw * sign;
}

}  // namespace vtd
