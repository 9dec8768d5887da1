// calib_kernels.hip — static intrinsic calibration (calico_camera_calibrate): the K intrinsics of a camera model jointly with
// the pose T_camera_chart of every frame of a ragged batch of (pixel, chart point) pairs, by Levenberg-Marquardt on the device.
//
// The arrowhead loop of arrowhead_dev.hpp, which describes the four launches of an iteration. What is this file's own: the border
// is the K x K block C of the intrinsics, which move additively (a held one has an identity row); a block of pairs is a frame, one
// wave per frame, kCalibWaves frames per workgroup; the rows are sqrt(w) [J_pose (6) | J_k (K) | e], N = K + 7 <= 18 columns (one
// accumulator tile, three for OpenCv8); the frame's share of the reduced system is C_f - B_f^T Y_f, its entries in calib_entry's
// order, summed in eight parts. The control word is CalibControl.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/calico_hip.h"
#include "arrowhead_dev.hpp"
#include "kernels.hpp"

namespace cal {

constexpr int kCalibWaves = 4;
constexpr int kCalibThreads = 64 * kCalibWaves;
constexpr int kCalibWavesPerSimd = 2;       // the register budget asked of the compiler: 256 VGPRs
constexpr int kCalibParts = 8;              // reduce: partial sums over the frames f = part (mod 8), added in order
constexpr int kCalibEntries = kCalibShare;  // reduce: entries summed (at most 66 + 11 + 11 + 4)
constexpr int kSlotCost = 7, kSlotSs = 8, kSlotValid = 9, kSlotNoise = 10;

namespace {

constexpr LmStatusCodes kCalibStatus = {CALICO_CALIB_OK, CALICO_CALIB_DEGENERATE, CALICO_CALIB_NOT_CONVERGED};

// The entries of a frame's share of the reduced system, in the order the reduction adds them up: the lower triangle of
// C_f - B_f^T Y_B by rows, then g_k - B_f^T Y_g (K), the diagonal of C_f (K: the damping's scale), then Sum rho, Sum |e|^2, the
// valid pairs and a one (the frames are counted). Entry el is  G[g_at] - (B^T Y)[s_row][s_col]  (g_at >= 0; s_row < 0: nothing
// to subtract), or the frame's slot value slot_at (>= 0), or 1.
DEV void calib_entry(int el, int K, int N, int* g_at, int* s_row, int* s_col, int* slot_at) {
  const int n_tri = K * (K + 1) / 2;
  *g_at = -1; *s_row = -1; *s_col = 0; *slot_at = -1;
  if (el < n_tri) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= el) ++i;
    const int j = el - i * (i + 1) / 2;
    *g_at = (6 + i) * N + 6 + j; *s_row = i; *s_col = j;
  } else if (el < n_tri + K) {
    const int i = el - n_tri;
    *g_at = (6 + i) * N + 6 + K; *s_row = i; *s_col = K;
  } else if (el < n_tri + 2 * K) {
    const int i = el - n_tri - K;
    *g_at = (6 + i) * N + 6 + i;
  } else if (el < n_tri + 2 * K + 3) {
    *slot_at = kSlotCost + (el - n_tri - 2 * K);      // kSlotCost, kSlotSs, kSlotValid
  }
}

}  // namespace

template <int MODEL>
__global__ __launch_bounds__(kCalibThreads, kCalibWavesPerSimd) void calib_evaluate_kernel(CalibArgs a) {
  constexpr int K = CamK<MODEL>::K, N = K + 7;
  constexpr bool kTwo = N > 16;
  __shared__ double s_x[kCalibWaves][64 * N];      // the wave's staging area: 64 rows of N columns
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t f = int64_t(blockIdx.x) * kCalibWaves + wave;
  if (f >= a.n_frames) return;      // (the whole wave: no barrier follows)
  const CalibControl* const c = a.ctrl;
  if (c->lm.done != 0 || c->lm.redo != 0 || a.active[f] == 0) return;
  const int cur = c->lm.cur, nxt = cur ^ 1;
  const bool first = c->lm.first != 0;
  double* const fr = a.frames + f * kCalibFrameDoubles;
  double* const ns = fr + kCalibSlot * nxt;
  const double* const k = c->k[nxt];
  // the candidate pose: wave-uniform, in registers
  Q4 q;
  V3 t;
  double step = 0.0;
  if (first) {
    q = slot_q(ns); t = slot_t(ns);
  } else {
    const double* const cs = fr + kCalibSlot * cur;
    double d[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double v = fr[kCalibY + 6 * K + r];
#pragma unroll
      for (int j = 0; j < K; ++j) v += fr[kCalibY + 6 * j + r] * c->dk[j];
      d[r] = -v;
    }
    step = retract_pose(slot_q(cs), slot_t(cs), mk(d[0], d[1], d[2]), mk(d[3], d[4], d[5]), &q, &t);
  }
  const M3 R = rotmat(q);
  const int64_t base = a.offsets[f], n = a.offsets[f + 1] - base;
  const double hs = a.huber_scale, hs2 = hs * hs;
  double* const X = s_x[wave];
  const int lc = lane & 15, lk = lane >> 4;
  // operand columns of this lane: lc of tile 0, 16 + lc of tile 1 (a column past N reads column 0 and is replaced by zero)
  const bool has1 = kTwo && 16 + lc < N;
  const double* const op0 = X + lk * N + (lc < N ? lc : 0);
  const double* const op1 = X + lk * N + (has1 ? 16 + lc : 0);
  f64x4 acc00 = {0, 0, 0, 0}, acc10 = {0, 0, 0, 0}, acc11 = {0, 0, 0, 0};
  double s_cost = 0.0, s_common = 0.0, s_ss = 0.0, s_noise = 0.0;
  int n_valid = 0, lost = 0;      // wave-uniform counts (ballots)
  for (int64_t i0 = 0; i0 < n; i0 += 64) {
    const int64_t i = base + i0 + lane;
    double x[2][N];
#pragma unroll
    for (int col = 0; col < N; ++col) { x[0][col] = 0.0; x[1][col] = 0.0; }
    bool ok = false, was = false;
    if (i0 + lane < n) {
      const V3 P = mk(a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2]);
      const double u = a.pixels[2 * i], v = a.pixels[2 * i + 1];
      const uint8_t fl = a.flags[i];
      was = !first && (fl & pose_bit(cur)) != 0;
      const V3 RP = mul(R, P), Pc = RP + t;
      double pix[2] = {0.0, 0.0}, D[2][3], dK[2][kMaxIntr];
      ok = project<MODEL, true>(k, Pc, pix, D, dK);
      ok = ok && __builtin_isfinite(pix[0]) && __builtin_isfinite(pix[1]);
      a.flags[i] = uint8_t((fl & ~pose_bit(nxt)) | (ok ? pose_bit(nxt) : 0));
      if (ok) {
        const double e[2] = {pix[0] - u, pix[1] - v}, sq = e[0] * e[0] + e[1] * e[1];
        double w, rho;
        huber(sq, hs, hs2, &w, &rho);
        const double sw = sqrt(w);
        // d Pc / d delta = -[R P]x: row r of J_pose is [(R P) x D_r, D_r]
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const V3 dd = mk(D[r][0], D[r][1], D[r][2]), cr = cross(RP, dd);
          x[r][0] = sw * cr.x; x[r][1] = sw * cr.y; x[r][2] = sw * cr.z; x[r][3] = sw * dd.x; x[r][4] = sw * dd.y; x[r][5] = sw * dd.z;
#pragma unroll
          for (int j = 0; j < K; ++j) x[r][6 + j] = ((a.free_bits >> j) & 1u) ? sw * dK[r][j] : 0.0;
          x[r][6 + K] = sw * e[r];
        }
        s_cost += rho; s_ss += sq; s_noise += dabs(e[0] * pix[0]) + dabs(e[1] * pix[1]);
        if (was) s_common += rho;
      }
    }
    n_valid += __popcll(__ballot(ok)); lost += __popcll(__ballot(was && !ok));
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      wave_fence();      // (the products of the previous rows have read the area)
#pragma unroll
      for (int col = 0; col < N; ++col) X[lane * N + col] = x[r][col];
      wave_fence();
#pragma unroll
      for (int g = 0; g < 2; ++g) {      // eight steps (32 rows) of operands at a time
        double v0[8], v1[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          v0[s] = op0[(32 * g + 4 * s) * N];
          if (kTwo) v1[s] = op1[(32 * g + 4 * s) * N];
        }
        if (lc >= N) {
#pragma unroll
          for (int s = 0; s < 8; ++s) v0[s] = 0.0;
        }
        if (kTwo && !has1) {
#pragma unroll
          for (int s = 0; s < 8; ++s) v1[s] = 0.0;
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(v0[s], v0[s], acc00, 0, 0, 0);
          if (kTwo) {
            acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(v1[s], v0[s], acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(v1[s], v1[s], acc11, 0, 0, 0);
          }
        }
      }
    }
  }
  gram_store<N>(a.gram + (f * 2 + nxt) * (N * N), lane, acc00, acc10, acc11);
  s_cost = wave_sum(s_cost); s_common = wave_sum(s_common); s_ss = wave_sum(s_ss); s_noise = wave_sum(s_noise);
  if (lane == 0) {
    put_slot_pose(ns, q, t);
    ns[kSlotCost] = s_cost; ns[kSlotSs] = s_ss; ns[kSlotValid] = double(n_valid); ns[kSlotNoise] = s_noise;
    fr[kCalibCommon] = s_common; fr[kCalibLost] = double(lost); fr[kCalibStep] = step;
  }
}

// One wave. The sums run over the frames that take part, lane l over l, l + 64, ..., then the wave sum: a fixed order.
__global__ __launch_bounds__(64) void calib_decide_kernel(CalibArgs a) {
  CalibControl* const c = a.ctrl;
  const int lane = threadIdx.x;
  if (c->lm.done != 0) return;
  if (c->lm.redo != 0) { if (lane == 0) c->lm.redo = 0; return; }
  const int cur = c->lm.cur, nxt = cur ^ 1;
  double cand = 0.0, common = 0.0, current = 0.0, noise = 0.0, lost = 0.0, valid = 0.0, step = 0.0;
  bool finite = true;
  // (no branch on the frame's flag: a frame that takes no part adds zero; its slots are finite, the host cleared them)
#pragma unroll 2
  for (int64_t f = lane; f < a.n_frames; f += 64) {
    const bool act = a.active[f] != 0;
    const double* const fr = a.frames + f * kCalibFrameDoubles;
    const double* const cs = fr + kCalibSlot * cur;
    const double* const ns = fr + kCalibSlot * nxt;
    const double v_cand = ns[kSlotCost], v_valid = ns[kSlotValid], v_common = fr[kCalibCommon], v_lost = fr[kCalibLost];
    const double v_current = cs[kSlotCost], v_noise = cs[kSlotNoise], v_step = fr[kCalibStep];
    const bool v_finite = finite_pose(slot_q(ns), slot_t(ns));
    cand += act ? v_cand : 0.0; valid += act ? v_valid : 0.0; common += act ? v_common : 0.0; lost += act ? v_lost : 0.0;
    current += act ? v_current : 0.0; noise += act ? v_noise : 0.0; step = fmax(step, act ? v_step : 0.0);
    finite = finite && (v_finite || !act);
  }
  cand = wave_sum(cand); common = wave_sum(common); current = wave_sum(current); noise = wave_sum(noise); lost = wave_sum(lost);
  valid = wave_sum(valid); step = wave_max(step);
  finite = __all(finite) != 0;
#pragma unroll 1
  for (int i = 0; i < a.K; ++i) finite = finite && __builtin_isfinite(c->k[nxt][i]);
  const bool kept = lost == 0.0 && finite && __builtin_isfinite(cand);
  const bool small = fmax(step, c->lm.step) < a.step_tolerance;
  lm_control_decide(&c->lm, lane, kept, valid >= 1.0, cand, common, current, noise, small, a.max_iterations, kCalibStatus);
}

// final: undamped, at the result, for every frame (the loop is over): the frame's outputs, Y and the share for the covariance.
__global__ __launch_bounds__(kCalibThreads) void calib_eliminate_kernel(CalibArgs a, int final) {
  __shared__ double s_w[kCalibWaves][36 + 6 * kMaxIntr];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t f = int64_t(blockIdx.x) * kCalibWaves + wave;
  if (f >= a.n_frames) return;
  const CalibControl* const c = a.ctrl;
  if (!final && c->lm.done != 0) return;
  const int K = a.K, N = K + 7, cur = c->lm.cur;
  double* const fr = a.frames + f * kCalibFrameDoubles;
  const double* const cs = fr + kCalibSlot * cur;
  bool active = a.active[f] != 0;
  if (active) {
    const double lambda = final ? 0.0 : c->lm.lambda;
    const double* const G = a.gram + (f * 2 + cur) * (N * N);
    double* const W = s_w[wave];
    double* const Y = W + 36;      // column j (K columns of B, then g) at 6 j
    if (lane < 36) { const int r = lane / 6, col = lane - 6 * r; W[lane] = G[r * N + col] * (r == col ? 1.0 + lambda : 1.0); }
    for (int e = lane; e < 6 * (K + 1); e += 64) { const int j = e / 6, r = e - 6 * j; Y[e] = G[r * N + 6 + j]; }
    wave_fence();
    if (!eliminate_frame_block(W, Y, K + 1, lane)) {
      active = false;
      if (lane == 0) { a.active[f] = 0; a.status[f] = uint8_t(final ? CALICO_RESECT_DEGENERATE : CALICO_RESECT_NOT_POSITIVE_DEFINITE); }
    } else {
      for (int e = lane; e < 6 * (K + 1); e += 64) fr[kCalibY + e] = Y[e];
      // the frame's share, entry by entry in the reduction's order: contiguous, so that the reduction's loads are whole lines
      double* const sh = a.share + f * kCalibEntries;
      const int n_el = K * (K + 1) / 2 + 2 * K + 4;
      for (int e = lane; e < n_el; e += 64) {
        int g_at, s_row, s_col, slot_at;
        calib_entry(e, K, N, &g_at, &s_row, &s_col, &slot_at);
        double v = 1.0;
        if (g_at >= 0) {
          v = G[g_at];
          if (s_row >= 0) v -= bty(G + 6 + s_row, N, Y + 6 * s_col);      // (B^T Y)[s_row][s_col]
        } else if (slot_at >= 0) {
          v = cs[slot_at];
        }
        sh[e] = v;
      }
    }
  }
  if (final && lane == 0) {
    put_pose_out(a.q_out + 4 * f, a.t_out + 3 * f, cs, active);
    a.rms_out[f] = active ? sqrt(cs[kSlotSs] / cs[kSlotValid]) : 0.0;
    a.n_used_out[f] = active ? int(cs[kSlotValid]) : 0;
  }
}

// One workgroup of kCalibParts x kCalibEntries threads: thread (part, entry) adds the entry (calib_entry) of the frames' shares,
// the loads of sixteen frames in flight at once.
__global__ __launch_bounds__(kCalibParts * kCalibEntries) void calib_reduce_kernel(CalibArgs a, int final) {
  __shared__ double s_part[kCalibParts][kCalibEntries];
  __shared__ double s_tot[kCalibEntries];
  __shared__ double s_S[kMaxIntr * kMaxIntr], s_Li[kMaxIntr * kMaxIntr], s_rhs[kMaxIntr];
  CalibControl* const c = a.ctrl;
  if (!final && c->lm.done != 0) return;      // (the whole workgroup)
  const int K = a.K, cur = c->lm.cur, nxt = cur ^ 1;
  const int n_tri = K * (K + 1) / 2, n_el = n_tri + 2 * K + 4;
  __builtin_assume(n_el <= kCalibEntries);      // (one trip)
  sum_shares<kCalibParts, kCalibEntries, 16>(a.share, kCalibEntries, a.active, a.n_frames, n_el, [](int) { return true; }, s_part, s_tot);
  if (threadIdx.x >= 64) return;      // the small system: wave 0
  const int lane = threadIdx.x;
  const double lambda = final ? 0.0 : c->lm.lambda;
  if (lane == 0) {
    for (int i = 0; i < K; ++i) {
      const bool fi = ((a.free_bits >> i) & 1u) != 0;
      for (int j = 0; j <= i; ++j) {
        const bool fj = ((a.free_bits >> j) & 1u) != 0;
        double v = s_tot[i * (i + 1) / 2 + j];
        if (i == j) v += lambda * s_tot[n_tri + K + i];
        s_S[i * K + j] = (fi && fj) ? v : (i == j ? 1.0 : 0.0);      // a constant: an identity row, a zero right-hand side
      }
      s_rhs[i] = fi ? -s_tot[n_tri + i] : 0.0;
    }
  }
  wave_fence();
  const bool pd = lds_chol(s_S, K, lane);
  if (!final) {
    if (!pd) { lm_control_not_pd(&c->lm, lane, lambda, CALICO_CALIB_DEGENERATE); return; }
    lds_chol_solve(s_S, s_rhs, K, lane);
    double step = 0.0;
#pragma unroll 1
    for (int i = 0; i < K; ++i) {
      const bool fi = ((a.free_bits >> i) & 1u) != 0;
      const double k0 = c->k[cur][i], d = fi ? s_rhs[i] : 0.0;
      double sz = dabs(d) / fmax(1.0, dabs(k0));
      if (!__builtin_isfinite(sz)) sz = 1e300;
      step = fmax(step, sz);
      if (lane == 0) { c->dk[i] = d; c->k[nxt][i] = fi ? k0 + d : k0; }
    }
    if (lane == 0) c->lm.step = step;
    return;
  }
  // the result: sums for the summary, and the covariance of the intrinsics, the inverse of the undamped reduced system
  const double cost = s_tot[n_tri + 2 * K], ss = s_tot[n_tri + 2 * K + 1], valid = s_tot[n_tri + 2 * K + 2], frames = s_tot[n_tri + 2 * K + 3];
  const double rms = sqrt(ss / valid);
  bool ok = pd && __builtin_isfinite(cost) && __builtin_isfinite(rms);
#pragma unroll 1
  for (int i = 0; i < K; ++i) ok = ok && __builtin_isfinite(c->k[cur][i]);
  chol_inverse_gram(s_S, s_Li, K, lane, [&](int e, int r, int col, double v) {
    const bool free_rc = ((a.free_bits >> r) & 1u) != 0 && ((a.free_bits >> col) & 1u) != 0;
    v = free_rc ? v : 0.0;
    ok = ok && __builtin_isfinite(v);
    if (a.cov_out) a.cov_out[e] = pd ? v : 0.0;
  });
  ok = __all(ok) != 0;
  lm_control_finish(&c->lm, lane, ok, cost, rms, frames, valid);
}

hipError_t launch_calib_evaluate(int model, const CalibArgs& a, hipStream_t s) {
  if (a.n_frames <= 0) return hipSuccess;
  const dim3 grid(unsigned((a.n_frames + kCalibWaves - 1) / kCalibWaves)), block(kCalibThreads);
  return with_camera_model(model, [&](auto m) { hipLaunchKernelGGL(calib_evaluate_kernel<decltype(m)::value>, grid, block, 0, s, a); });
}
hipError_t launch_calib_decide(const CalibArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(calib_decide_kernel, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_calib_eliminate(const CalibArgs& a, bool final, hipStream_t s) {
  if (a.n_frames <= 0) return hipSuccess;
  const dim3 grid(unsigned((a.n_frames + kCalibWaves - 1) / kCalibWaves)), block(kCalibThreads);
  hipLaunchKernelGGL(calib_eliminate_kernel, grid, block, 0, s, a, final ? 1 : 0);
  return hipGetLastError();
}
hipError_t launch_calib_reduce(const CalibArgs& a, bool final, hipStream_t s) {
  hipLaunchKernelGGL(calib_reduce_kernel, dim3(1), dim3(kCalibParts * kCalibEntries), 0, s, a, final ? 1 : 0);
  return hipGetLastError();
}

}  // namespace cal
