// rig.cpp — calico_rig_calibrate (this part of the C ABI of include/calico_hip.h): the extrinsics of the cameras of a rig and
// the pose of every rig frame from shared chart views (rig_kernels.hip), started from a resection of every view
// (resect_kernels.hip) and, on the host, a breadth-first tree over the cameras that share frames. The views are sorted by
// (frame, camera) before anything is summed, and the outputs per view go back in the caller's order. What can be checked without
// a device is checked before the first HIP call (arg_rules.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/calico_hip.h"
#include "arg_rules.hpp"
#include "free_call.hpp"
#include "kernels.hpp"
#include "lm_host.hpp"
#include "lm_rule.hpp"

namespace {

using namespace cal;

static_assert(kRigMaxCameras == CALICO_RIG_MAX_CAMERAS, "the kernels' table of cameras is the header's");

// a rigid transform: unit quaternion (x, y, z, w) and translation
struct Pose { double q[4] = {0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0}; };

void quat_mul(const double* a, const double* b, double* r) {      // R(a b) = R(a) R(b)
  const double x = a[3] * b[0] + b[3] * a[0] + a[1] * b[2] - a[2] * b[1];
  const double y = a[3] * b[1] + b[3] * a[1] + a[2] * b[0] - a[0] * b[2];
  const double z = a[3] * b[2] + b[3] * a[2] + a[0] * b[1] - a[1] * b[0];
  const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  r[0] = x; r[1] = y; r[2] = z; r[3] = w;
}
void rotate(const double* q, const double* v, double* r) {      // R(q) v, q unit
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2.0 * (y * v[2] - z * v[1]), ty = 2.0 * (z * v[0] - x * v[2]), tz = 2.0 * (x * v[1] - y * v[0]);
  const double rx = v[0] + w * tx + (y * tz - z * ty), ry = v[1] + w * ty + (z * tx - x * tz), rz = v[2] + w * tz + (x * ty - y * tx);
  r[0] = rx; r[1] = ry; r[2] = rz;
}
Pose compose(const Pose& a, const Pose& b) {      // a b
  Pose r;
  double q[4];
  quat_mul(a.q, b.q, q);
  canonical_unit_quat(q, quat_norm(q), r.q);
  rotate(a.q, b.t, r.t);
  for (int i = 0; i < 3; ++i) r.t[i] += a.t[i];
  return r;
}
Pose inverse(const Pose& a) {
  Pose r;
  r.q[0] = -a.q[0]; r.q[1] = -a.q[1]; r.q[2] = -a.q[2]; r.q[3] = a.q[3];
  double t[3];
  rotate(r.q, a.t, t);
  for (int i = 0; i < 3; ++i) r.t[i] = -t[i];
  return r;
}
// The mean of transforms: the chordal mean of the rotations (the dominant eigenvector of Sum q q^T, by power iteration from the
// first sample: the samples of one edge lie within a few degrees of each other), the mean of the translations. Sums in the order given.
Pose mean_pose(const std::vector<Pose>& samples) {
  double A[4][4] = {}, t[3] = {};
  for (const Pose& s : samples) {
    double d = 0.0;
    for (int i = 0; i < 4; ++i) d += s.q[i] * samples[0].q[i];
    const double sg = d < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) A[i][j] += (sg * s.q[i]) * (sg * s.q[j]);
    for (int i = 0; i < 3; ++i) t[i] += s.t[i];
  }
  double v[4] = {samples[0].q[0], samples[0].q[1], samples[0].q[2], samples[0].q[3]};
  for (int it = 0; it < 64; ++it) {
    double w[4] = {};
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) w[i] += A[i][j] * v[j];
    const double n = quat_norm(w);
    if (!(n > 0.0)) break;
    for (int i = 0; i < 4; ++i) v[i] = w[i] / n;
  }
  Pose r;
  canonical_unit_quat(v, quat_norm(v), r.q);
  for (int i = 0; i < 3; ++i) r.t[i] = t[i] / double(samples.size());
  return r;
}

}  // namespace

extern "C" {

// max_iterations, step_tolerance, huber_scale, min_points, min_shared_frames, reference_camera
void calico_default_rig_options(calico_rig_options* o) { if (o) *o = {50, 1e-10, 0.0, 4, 3, 0}; }

int32_t calico_rig_calibrate(int32_t device, int32_t n_cameras, const int32_t* models, const int64_t* intrinsics_offsets,
                             const double* intrinsics, int64_t n_frames, int64_t n_views, const int32_t* view_camera,
                             const int64_t* view_frame, const int64_t* view_offsets, const double* pixels, const double* points,
                             const double* q_rig_camera_init, const double* t_rig_camera_init, const double* q_frame_init,
                             const double* t_frame_init, const calico_rig_options* opt, double* q_rig_camera_out,
                             double* t_rig_camera_out, uint8_t* camera_status_out, double* q_frame_out, double* t_frame_out,
                             uint8_t* frame_status_out, double* view_rms_out, int32_t* view_n_used_out, uint8_t* view_status_out,
                             double* extrinsics_cov_out, calico_rig_summary* summary) {
  const FreeCall call{"calico_rig_calibrate"};
  calico_rig_options o;
  calico_default_rig_options(&o);
  if (opt) o = *opt;
  int num_params[kRigMaxCameras] = {};
  if (models && n_cameras >= 1 && n_cameras <= kRigMaxCameras)
    for (int c = 0; c < n_cameras; ++c) num_params[c] = camera_model_num_params(models[c]);
  std::string error = rig_cameras_error(n_cameras, kRigMaxCameras, models, num_params, intrinsics_offsets, intrinsics);
  if (error.empty()) error = rig_options_error(n_cameras, n_frames, n_views, o, q_rig_camera_init, t_rig_camera_init, q_frame_init, t_frame_init);
  if (error.empty() && !(q_rig_camera_out && t_rig_camera_out && camera_status_out && summary)) error = "null camera output buffer or summary";
  if (error.empty() && n_frames > 0 && !(q_frame_out && t_frame_out && frame_status_out)) error = "null frame output buffer";
  if (error.empty() && n_views > 0 && !(view_rms_out && view_n_used_out && view_status_out)) error = "null view output buffer";
  std::vector<int64_t> order(size_t(std::max<int64_t>(n_views, 0)));
  if (error.empty() && n_views > 0)
    error = rig_views_error(n_cameras, n_frames, n_views, view_camera, view_frame, view_offsets, pixels, points, order.data());
  if (!error.empty()) return call.invalid(error);

  const int C = n_cameras, M = 6 * C, ref = o.reference_camera;
  const size_t F = size_t(n_frames), V = size_t(n_views);
  // the start of the cameras (as the device takes it) and, where the caller gave one, of the frames
  std::vector<Pose> cam(size_t(C), Pose{}), frame(F);
  if (q_rig_camera_init)
    for (int c = 0; c < C; ++c) {
      canonical_unit_quat(q_rig_camera_init + 4 * c, quat_norm(q_rig_camera_init + 4 * c), cam[size_t(c)].q);
      std::copy(t_rig_camera_init + 3 * c, t_rig_camera_init + 3 * c + 3, cam[size_t(c)].t);
    }
  if (q_frame_init)
    for (size_t f = 0; f < F; ++f) {
      canonical_unit_quat(q_frame_init + 4 * f, quat_norm(q_frame_init + 4 * f), frame[f].q);
      std::copy(t_frame_init + 3 * f, t_frame_init + 3 * f + 3, frame[f].t);
    }
  std::vector<uint8_t> cam_status(size_t(C), uint8_t(CALICO_RIG_CAMERA_UNCONNECTED)), frame_status(F, uint8_t(CALICO_RIG_FRAME_NO_VIEW));
  cam_status[size_t(ref)] = CALICO_RIG_CAMERA_REFERENCE;
  std::vector<uint8_t> vstat(V, uint8_t(CALICO_RESECT_OK));      // per view, sorted order
  // the outputs that are the starts (too few views, a degenerate problem); a held camera's are its start as given
  const auto give_starts = [&](int status, int iterations, double lambda, bool held_only) {
    for (int c = 0; c < C; ++c) {
      if (held_only && cam_status[size_t(c)] == CALICO_RIG_CAMERA_OK) continue;
      const bool raw = q_rig_camera_init && cam_status[size_t(c)] != CALICO_RIG_CAMERA_OK;
      for (int i = 0; i < 4; ++i) q_rig_camera_out[4 * c + i] = raw ? q_rig_camera_init[4 * c + i] : cam[size_t(c)].q[i];
      for (int i = 0; i < 3; ++i) t_rig_camera_out[3 * c + i] = raw ? t_rig_camera_init[3 * c + i] : cam[size_t(c)].t[i];
    }
    std::copy(cam_status.begin(), cam_status.end(), camera_status_out);
    if (held_only) return;
    for (size_t f = 0; f < F; ++f) {
      std::copy(frame[f].q, frame[f].q + 4, q_frame_out + 4 * f); std::copy(frame[f].t, frame[f].t + 3, t_frame_out + 3 * f);
      frame_status_out[f] = frame_status[f];
    }
    for (size_t s = 0; s < V; ++s) {
      const size_t v = size_t(order[s]);
      view_rms_out[v] = 0.0; view_n_used_out[v] = 0; view_status_out[v] = vstat[s];
    }
    if (extrinsics_cov_out) std::fill(extrinsics_cov_out, extrinsics_cov_out + size_t(M) * size_t(M), 0.0);
    *summary = calico_rig_summary{};
    summary->status = status; summary->iterations = iterations; summary->lambda = lambda;
    for (int c = 0; c < C; ++c) summary->cameras_used += cam_status[size_t(c)] != CALICO_RIG_CAMERA_UNCONNECTED ? 1 : 0;
    for (size_t f = 0; f < F; ++f) summary->frames_used += frame_status[f] == CALICO_RIG_FRAME_OK ? 1 : 0;
  };
  if (n_views == 0) { give_starts(CALICO_RIG_TOO_FEW_VIEWS, 0, kLmLambda0, false); return CALICO_OK; }
  if (int rc = call.select_device(device)) return rc;

  // the views in (frame, camera) order, their pairs packed in that order
  const size_t P = size_t(view_offsets[n_views]);
  std::vector<int> s_cam(V);
  std::vector<int64_t> s_frame(V), s_off(V + 1, 0), frame_views(F + 1, 0);
  std::vector<double> s_px(P * 2), s_pt(P * 3);
  for (size_t s = 0; s < V; ++s) {
    const size_t v = size_t(order[s]);
    const int64_t b = view_offsets[v], n = view_offsets[v + 1] - b;
    s_cam[s] = view_camera[v]; s_frame[s] = view_frame[v]; s_off[s + 1] = s_off[s] + n;
    std::copy(pixels + 2 * b, pixels + 2 * (b + n), s_px.begin() + 2 * s_off[s]);
    std::copy(points + 3 * b, points + 3 * (b + n), s_pt.begin() + 3 * s_off[s]);
    ++frame_views[size_t(s_frame[s]) + 1];
  }
  for (size_t f = 0; f < F; ++f) frame_views[f + 1] += frame_views[f];

  // which views are usable, and T_camera_chart of each where the frames have no start
  std::vector<Pose> view_pose(V);
  if (q_frame_init) {
    for (size_t s = 0; s < V; ++s)
      if (s_off[s + 1] - s_off[s] < o.min_points) vstat[s] = CALICO_RESECT_TOO_FEW_POINTS;
  } else {
    calico_resection_options ro;
    calico_default_resection_options(&ro);
    ro.huber_scale = o.huber_scale; ro.min_points = o.min_points;
    for (int c = 0; c < C; ++c) {      // camera c's views: one batch of the resection, in frame order
      std::vector<size_t> mine;
      std::vector<int64_t> off(1, 0);
      for (size_t s = 0; s < V; ++s)
        if (s_cam[s] == c) { mine.push_back(s); off.push_back(off.back() + (s_off[s + 1] - s_off[s])); }
      if (mine.empty()) continue;
      const size_t nf = mine.size(), np = size_t(off.back());
      std::vector<double> px(np * 2), pt(np * 3), q(nf * 4), t(nf * 3);
      std::vector<uint8_t> st(nf);
      for (size_t i = 0; i < nf; ++i) {
        const size_t s = mine[i];
        std::copy(s_px.begin() + 2 * s_off[s], s_px.begin() + 2 * s_off[s + 1], px.begin() + 2 * off[i]);
        std::copy(s_pt.begin() + 3 * s_off[s], s_pt.begin() + 3 * s_off[s + 1], pt.begin() + 3 * off[i]);
      }
      FreeBuf<double> d_k, d_px, d_pt;
      FreeBuf<int64_t> d_off;
      FreeBuf<uint8_t> d_fl;
      ResectRun run;
      FREE_TRY(call, d_k.upload(intrinsics + intrinsics_offsets[c], size_t(num_params[c])));
      FREE_TRY(call, d_px.upload(px.data(), np * 2)); FREE_TRY(call, d_pt.upload(pt.data(), np * 3));
      FREE_TRY(call, d_fl.alloc(np)); FREE_TRY(call, d_fl.zero(np)); FREE_TRY(call, d_off.upload(off.data(), nf + 1));
      FREE_TRY(call, run.alloc(nf, np, false));
      FREE_TRY(call, run.start(models[c], ro, d_k.p, nf, d_off.p, d_px.p, d_pt.p, d_fl.p, q.data(), t.data(), st.data()));
      for (size_t i = 0; i < nf; ++i) {
        vstat[mine[i]] = st[i];
        std::copy(&q[4 * i], &q[4 * i] + 4, view_pose[mine[i]].q); std::copy(&t[3 * i], &t[3 * i] + 3, view_pose[mine[i]].t);
      }
    }
  }

  // the cameras that share frames: a breadth-first tree from the reference camera, neighbours in index order
  std::vector<int> shared(size_t(C) * size_t(C), 0), parent(size_t(C), -1), bfs(1, ref);
  for (size_t f = 0; f < F; ++f)
    for (int64_t s1 = frame_views[f]; s1 < frame_views[f + 1]; ++s1)
      for (int64_t s2 = frame_views[f]; s2 < frame_views[f + 1]; ++s2)
        if (s1 != s2 && vstat[size_t(s1)] == CALICO_RESECT_OK && vstat[size_t(s2)] == CALICO_RESECT_OK)
          ++shared[size_t(s_cam[size_t(s1)]) * size_t(C) + size_t(s_cam[size_t(s2)])];
  for (size_t head = 0; head < bfs.size(); ++head) {
    const int a = bfs[head];
    for (int b = 0; b < C; ++b) {
      if (cam_status[size_t(b)] != CALICO_RIG_CAMERA_UNCONNECTED || shared[size_t(a) * size_t(C) + size_t(b)] < o.min_shared_frames) continue;
      cam_status[size_t(b)] = CALICO_RIG_CAMERA_OK; parent[size_t(b)] = a; bfs.push_back(b);
      if (q_rig_camera_init) continue;
      std::vector<Pose> samples;      // T_a_b per shared frame, in frame order
      for (size_t f = 0; f < F; ++f) {
        int64_t sa = -1, sb = -1;
        for (int64_t s = frame_views[f]; s < frame_views[f + 1]; ++s) {
          if (vstat[size_t(s)] != CALICO_RESECT_OK) continue;
          if (s_cam[size_t(s)] == a) sa = s;
          if (s_cam[size_t(s)] == b) sb = s;
        }
        if (sa >= 0 && sb >= 0) samples.push_back(compose(view_pose[size_t(sa)], inverse(view_pose[size_t(sb)])));
      }
      cam[size_t(b)] = compose(cam[size_t(a)], mean_pose(samples));
    }
  }
  // who takes part; a frame starts from its usable view of lowest camera index
  std::vector<uint8_t> view_active(V, 0), view_writer(V, 0), frame_active(F, 0);
  unsigned held_bits = 0;
  int connected = 0;
  for (int c = 0; c < C; ++c) {
    if (cam_status[size_t(c)] != CALICO_RIG_CAMERA_OK) held_bits |= 1u << c;
    else ++connected;
  }
  for (size_t s = 0; s < V; ++s) {
    const size_t f = size_t(s_frame[s]);
    view_active[s] = vstat[s] == CALICO_RESECT_OK && cam_status[size_t(s_cam[s])] != CALICO_RIG_CAMERA_UNCONNECTED ? 1 : 0;
    if (!view_active[s] || frame_active[f]) continue;
    frame_active[f] = 1; view_writer[s] = 1; frame_status[f] = CALICO_RIG_FRAME_OK;
    if (!q_frame_init) frame[f] = compose(cam[size_t(s_cam[s])], view_pose[s]);
  }
  for (size_t f = 0; f < F; ++f)
    if (!frame_active[f]) frame[f] = Pose{};
  if (connected == 0) { give_starts(CALICO_RIG_TOO_FEW_VIEWS, 0, kLmLambda0, false); return CALICO_OK; }

  // the device's state
  std::vector<std::vector<int>> lists(8);      // per camera model: its active views
  for (size_t s = 0; s < V; ++s)
    if (view_active[s]) lists[size_t(models[s_cam[s]])].push_back(int(s));
  FreeBuf<double> d_k, d_px, d_pt, d_frames, d_views, d_gram, d_share, d_q, d_t, d_rms, d_cov;
  FreeBuf<int64_t> d_vframe, d_voff, d_fviews;
  FreeBuf<int32_t> d_vcam, d_used, d_lists[8];
  FreeBuf<uint8_t> d_fl, d_vact, d_vwr, d_fact, d_fst;
  FreeBuf<RigControl> d_ctrl;
  FREE_TRY(call, d_k.upload(intrinsics, size_t(intrinsics_offsets[C]))); FREE_TRY(call, d_px.upload(s_px.data(), P * 2));
  FREE_TRY(call, d_pt.upload(s_pt.data(), P * 3)); FREE_TRY(call, d_fl.alloc(P)); FREE_TRY(call, d_fl.zero(P));
  FREE_TRY(call, d_vcam.upload(s_cam.data(), V)); FREE_TRY(call, d_vframe.upload(s_frame.data(), V)); FREE_TRY(call, d_voff.upload(s_off.data(), V + 1));
  FREE_TRY(call, d_fviews.upload(frame_views.data(), F + 1)); FREE_TRY(call, d_vact.upload(view_active.data(), V));
  FREE_TRY(call, d_vwr.upload(view_writer.data(), V)); FREE_TRY(call, d_fact.upload(frame_active.data(), F));
  FREE_TRY(call, d_fst.upload(frame_status.data(), F));
  for (int m = 1; m < 8; ++m) FREE_TRY(call, d_lists[m].upload(lists[size_t(m)].data(), lists[size_t(m)].size()));
  std::vector<double> frames(F * kRigFrameDoubles, 0.0);
  for (size_t f = 0; f < F; ++f)      // the start is the candidate of the first evaluation: slot 1 (slot 0 holds it too: finite)
    for (int slot = 0; slot < 2; ++slot) {
      double* ns = frames.data() + f * kRigFrameDoubles + 8 * slot;
      std::copy(frame[f].q, frame[f].q + 4, ns); std::copy(frame[f].t, frame[f].t + 3, ns + 4);
    }
  RigControl ctrl = {};
  ctrl.lm.status = CALICO_RIG_NOT_CONVERGED; ctrl.lm.first = 1; ctrl.lm.lambda = kLmLambda0;
  for (int slot = 0; slot < 2; ++slot)
    for (int c = 0; c < C; ++c) {
      std::copy(cam[size_t(c)].q, cam[size_t(c)].q + 4, ctrl.cam[slot][c]); std::copy(cam[size_t(c)].t, cam[size_t(c)].t + 3, ctrl.cam[slot][c] + 4);
    }
  FREE_TRY(call, d_frames.upload(frames.data(), frames.size())); FREE_TRY(call, d_ctrl.upload(&ctrl, 1));
  FREE_TRY(call, d_views.alloc(V * kRigViewDoubles)); FREE_TRY(call, d_views.zero(V * kRigViewDoubles));
  FREE_TRY(call, d_gram.alloc(V * 2 * kRigN * kRigN)); FREE_TRY(call, d_gram.zero(V * 2 * kRigN * kRigN));
  FREE_TRY(call, d_share.alloc(F * kRigShare)); FREE_TRY(call, d_share.zero(F * kRigShare));
  FREE_TRY(call, d_q.alloc(F * 4)); FREE_TRY(call, d_t.alloc(F * 3)); FREE_TRY(call, d_rms.alloc(V)); FREE_TRY(call, d_used.alloc(V));
  FREE_TRY(call, d_cov.alloc(size_t(M) * size_t(M)));

  RigArgs a = {};
  a.ctrl = d_ctrl.p; a.n_cameras = C; a.held_bits = held_bits; a.intrinsics = d_k.p; a.n_frames = n_frames; a.n_views = n_views;
  for (int c = 0; c < C; ++c) a.intr_at[c] = int(intrinsics_offsets[c]);
  a.view_camera = d_vcam.p; a.view_frame = d_vframe.p; a.view_offsets = d_voff.p; a.frame_views = d_fviews.p; a.pixels = d_px.p; a.points = d_pt.p;
  a.flags = d_fl.p; a.view_active = d_vact.p; a.view_writer = d_vwr.p; a.frame_active = d_fact.p; a.frame_status = d_fst.p;
  a.frames = d_frames.p; a.views = d_views.p; a.gram = d_gram.p; a.share = d_share.p;
  a.max_iterations = o.max_iterations; a.step_tolerance = o.step_tolerance; a.huber_scale = o.huber_scale;
  a.q_frame_out = d_q.p; a.t_frame_out = d_t.p; a.view_rms_out = d_rms.p; a.view_n_used_out = d_used.p; a.cov_out = d_cov.p;
  const int rc = run_device_lm(call, &d_ctrl.p->lm.done, o.max_iterations, [&] {
    hipError_t e = hipSuccess;
    for (int m = 1; m < 8 && e == hipSuccess; ++m) e = launch_rig_evaluate(m, a, d_lists[m].p, int(lists[size_t(m)].size()), nullptr);
    if (e == hipSuccess) e = launch_rig_decide(a, nullptr);
    if (e == hipSuccess) e = launch_rig_eliminate(a, false, nullptr);
    return e != hipSuccess ? e : launch_rig_reduce(a, false, nullptr);
  });
  if (rc != CALICO_OK) return rc;
  FREE_TRY(call, d_ctrl.download(&ctrl, 1));
  const LmControl& lm = ctrl.lm;
  if (lm.status != CALICO_RIG_DEGENERATE) {
    FREE_TRY(call, launch_rig_eliminate(a, true, nullptr)); FREE_TRY(call, launch_rig_reduce(a, true, nullptr));
    FREE_TRY(call, d_ctrl.download(&ctrl, 1));
  }
  if (lm.status == CALICO_RIG_DEGENERATE || !lm.final_ok) {
    give_starts(CALICO_RIG_DEGENERATE, lm.iterations, lm.lambda, false);
    return CALICO_OK;
  }
  give_starts(lm.status, 0, 0.0, true);      // the held cameras, every camera's status
  for (int c = 0; c < C; ++c) {
    if (cam_status[size_t(c)] != CALICO_RIG_CAMERA_OK) continue;
    std::copy(ctrl.cam[lm.cur][c], ctrl.cam[lm.cur][c] + 4, q_rig_camera_out + 4 * c);
    std::copy(ctrl.cam[lm.cur][c] + 4, ctrl.cam[lm.cur][c] + 7, t_rig_camera_out + 3 * c);
  }
  FREE_TRY(call, d_q.download(q_frame_out, F * 4)); FREE_TRY(call, d_t.download(t_frame_out, F * 3));
  FREE_TRY(call, d_fst.download(frame_status_out, F));
  std::vector<double> rms(V);
  std::vector<int32_t> used(V);
  FREE_TRY(call, d_rms.download(rms.data(), V)); FREE_TRY(call, d_used.download(used.data(), V));
  for (size_t s = 0; s < V; ++s) {
    const size_t v = size_t(order[s]);
    view_rms_out[v] = rms[s]; view_n_used_out[v] = used[s]; view_status_out[v] = vstat[s];
  }
  if (extrinsics_cov_out) FREE_TRY(call, d_cov.download(extrinsics_cov_out, size_t(M) * size_t(M)));
  *summary = calico_rig_summary{};
  summary->status = lm.status; summary->iterations = lm.iterations; summary->initial_cost = lm.initial_cost;
  summary->final_cost = lm.final_cost; summary->rms = lm.rms; summary->cameras_used = connected + 1;
  summary->frames_used = lm.frames_used; summary->views_used = ctrl.views_used; summary->pairs_used = lm.pairs_used;
  summary->lambda = lm.lambda;
  return CALICO_OK;
}

}  // extern "C"
