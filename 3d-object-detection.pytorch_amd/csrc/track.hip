// The demo's IOU tracker as a device-resident stage (include/t3d.h: t3d_track_step; reference torchdet3d/utils/
// tracking_tools.py:127-290 `IOUTracker`, :9-124 `Track`; call site scripts/demo.py:56-78).
//
// One workgroup of ONE wave per stream: a frame's work is a chain of short dependent steps (active list -> cost matrix ->
// augmenting paths -> per-track updates -> id hand-out -> compaction), each a few dozen items wide at the sizes the detector
// produces (<= 64 detections, a handful of tracks); a single wave needs no cross-wave barrier between them and the launch is
// latency-bound, not throughput-bound.  Streams (cameras) are independent and go to separate workgroups.
//
// The tracker state lives in device memory between launches (layout: StateView below; all zero = a fresh tracker) and is
// worked on in place; LDS holds what the frame itself needs: the detections' boxes, the fp32 cost matrix and the
// assignment's potentials / labels.  The table of tracks is bounded (max_tracks): every index into it is < T by
// construction (a track is appended only while num_tracks < T, compaction only moves towards the front), detections beyond
// `max_dets` are never read (counts are clamped), and a state whose counters are out of range is clamped on load.
//
// Arithmetic follows the reference's Python literally: box and area arithmetic in integers, every quotient and the EMAs in
// fp64 with product and sum rounded separately (the library is built with -ffp-contract=off), int() as truncation towards
// zero.  Keypoints are fp64 throughout (the reference's float32 corners -- a new track's first update, interpolated
// entries -- differ by a few 2^-24).
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int kLanes = 64;
constexpr int kMaxLds = 160 * 1024;      // LDS a single workgroup can have on gfx950
enum { H_TIME = 0, H_NUM = 1, H_LAST_ID = 2, H_DROPPED = 3, H_CLEARED = 4, H_RING_HEAD = 5, H_RING_COUNT = 6, H_WORDS = 8 };

struct TrackParams {
  int time_window, continue_thresh, clear_thresh, nouf_thresh, align_kp;
  double match_thr, iou_thr, box_speed, kp_speed, add_thr;
};

struct TrackArgs {
  unsigned char* state;
  long long state_stride;
  const int* dets;
  const float* kps;
  const int* counts;
  int D, T;
  TrackParams p;
  int* out_count;
  int* out_boxes;
  double* out_kp;
  int* out_ids;
  int* out_scalars;
};

// per stream: header words, then one array per field (T entries each); `ring` is the FIFO of released ids -- an id is only
// minted while the ring is empty, so ring entries + live tracks <= T at all times and T entries are enough
struct StateView {
  int* hdr;
  double* kp;      // [T][18]
  int* box;        // [T][4]
  int* id;
  int* end;        // time stamp of the last entry
  int* len;        // number of entries (interpolated ones included)
  int* nouf;       // no_updated_frames
  int* ring;
};
__host__ __device__ inline long long state_bytes(int T) {
  return ((long long)H_WORDS * 4 + (long long)T * (18 * 8 + 4 * 4 + 5 * 4) + 15) / 16 * 16;
}
__device__ inline StateView state_view(unsigned char* base, int T) {
  StateView s;
  s.hdr = reinterpret_cast<int*>(base);
  s.kp = reinterpret_cast<double*>(base + H_WORDS * 4);
  s.box = reinterpret_cast<int*>(s.kp + (size_t)T * 18);
  s.id = s.box + (size_t)T * 4;
  s.end = s.id + T;
  s.len = s.end + T;
  s.nouf = s.len + T;
  s.ring = s.nouf + T;
  return s;
}

// LDS carve: doubles first, then 4-byte arrays; every section a multiple of 8 bytes
struct LdsPlan { int off_u, off_v, off_minv, off_cost, off_p, off_way, off_used, off_act, off_assign, off_dbox, off_slot, off_newid, off_sh, total; };
__host__ __device__ inline LdsPlan lds_plan(int D, int T) {
  const int Me = ((D > T ? D : T) + 2) & ~1;      // + the virtual column 0, rounded up to even
  const int De = (D + 1) & ~1, Te = (T + 1) & ~1;
  LdsPlan l;
  int o = 0;
  l.off_u = o; o += Me * 8;
  l.off_v = o; o += Me * 8;
  l.off_minv = o; o += Me * 8;
  l.off_cost = o; o += ((D * T + 1) & ~1) * 4;
  l.off_p = o; o += Me * 4;
  l.off_way = o; o += Me * 4;
  l.off_used = o; o += Me * 4;
  l.off_act = o; o += Te * 4;
  l.off_assign = o; o += De * 4;
  l.off_dbox = o; o += De * 16;
  l.off_slot = o; o += De * 4;
  l.off_newid = o; o += De * 4;
  l.off_sh = o; o += 8 * 4;
  l.total = (o + 15) / 16 * 16;
  return l;
}
__host__ inline long long lds_bytes_ll(int D, int T) {
  const long long M = (D > T ? D : T) + 2;
  return M * 36 + (long long)D * T * 4 + (long long)T * 4 + (long long)D * 28 + 128;    // >= lds_plan().total, no int overflow
}

// tracking_tools.py:263-290 on integer boxes (64-bit: the products of pixel extents)
__device__ inline long long box_area(long long l, long long t, long long r, long long b) {
  const long long w = r - l, h = b - t;
  return (w > 0 ? w : 0) * (h > 0 ? h : 0);
}
__device__ inline void box_terms(const int* b1, const int* b2, long long& inter, long long& enclosing, long long& u) {
  inter = box_area(max(b1[0], b2[0]), max(b1[1], b2[1]), min(b1[2], b2[2]), min(b1[3], b2[3]));
  enclosing = box_area(min(b1[0], b2[0]), min(b1[1], b2[1]), max(b1[2], b2[2]), max(b1[3], b2[3]));
  u = box_area(b1[0], b1[1], b1[2], b1[3]) + box_area(b2[0], b2[1], b2[2], b2[3]) - inter;
}
__device__ inline double box_iou(const int* b1, const int* b2) {
  long long inter, enclosing, u;
  box_terms(b1, b2, inter, enclosing, u);
  return u > 0 ? (double)inter / (double)u : 0.0;
}
__device__ inline double box_giou(const int* b1, const int* b2) {
  long long inter, enclosing, u;
  box_terms(b1, b2, inter, enclosing, u);
  const double iou = u > 0 ? (double)inter / (double)u : 0.0;
  return enclosing > 0 ? iou - (double)(enclosing - u) / (double)enclosing : -1.0;
}

__device__ inline double kp_dist(const double* a, const double* b) {
  const double dx = a[0] - b[0], dy = a[1] - b[1];
  return sqrt(dx * dx + dy * dy);
}
__device__ inline double kp_mean_dist(const double* a, const double* b) {
  double s = 0.0;
  for (int k = 0; k < 9; ++k) s += kp_dist(a + 2 * k, b + 2 * k);
  return s / 9.0;
}

// Track.add_detection (tracking_tools.py:112-124) for track t and detection (nb, nk) at `time`
__device__ void add_detection(const StateView& st, int t, const int* nb, const double* nk, int time, const TrackParams& p) {
  const int skip = time - st.end[t];
  int pb[4];
  double pk[18];
  for (int c = 0; c < 4; ++c) pb[c] = st.box[4 * t + c];
  for (int k = 0; k < 18; ++k) pk[k] = st.kp[18 * (size_t)t + k];
  int len = st.len[t];
  bool filtered = skip == 1;
  if (skip > 1 && skip <= p.continue_thresh) {
    // _interpolate (:33-41): entries t = 1 .. skip-1 between the last box and the new one; only the last is read afterwards
    const double sk = (double)skip, tt = (double)(skip - 1);
    for (int c = 0; c < 4; ++c) pb[c] = (int)((double)pb[c] + (double)((long long)nb[c] - pb[c]) / sk * tt);
    for (int k = 0; k < 18; ++k) pk[k] = pk[k] + (nk[k] - pk[k]) / sk * tt;
    len += skip - 1;
    filtered = true;
  }
  st.len[t] = len + 1;
  st.end[t] = time;
  if (!filtered) {      // (a gap the interpolation does not bridge: the filters' `timestamps[-1] - timestamps[-2] == 1` fails)
    for (int c = 0; c < 4; ++c) st.box[4 * t + c] = nb[c];
    for (int k = 0; k < 18; ++k) st.kp[18 * (size_t)t + k] = nk[k];
    return;
  }
  // _filter_last_box (:104-110)
  for (int c = 0; c < 4; ++c) st.box[4 * t + c] = (int)((1.0 - p.box_speed) * (double)pb[c] + p.box_speed * (double)nb[c]);
  // _filter_last_3d_box (:43-75)
  double ck[18];
  for (int k = 0; k < 18; ++k) ck[k] = nk[k];
  double dist = kp_mean_dist(nk, pk);
  if (p.align_kp) {
    // _align_kp_positions (:77-102), literally: `distance` is not updated inside the inner loop, so the LAST j closer than
    // the keypoint's own previous position wins
    int idx[9];
    bool done[9];
    for (int i = 0; i < 9; ++i) { idx[i] = i; done[i] = false; }
    for (int i = 0; i < 9; ++i) {
      if (done[i]) continue;
      const double distance = kp_dist(nk + 2 * i, pk + 2 * i);
      int best = i;
      for (int j = i + 1; j < 9; ++j)
        if (kp_dist(nk + 2 * i, pk + 2 * j) < distance) best = j;
      if (best != i && !done[best]) {
        idx[i] = best;
        idx[best] = i;
        done[i] = done[best] = true;
      }
    }
    double sw[18];
    for (int i = 0; i < 9; ++i) { sw[2 * i] = nk[2 * idx[i]]; sw[2 * i + 1] = nk[2 * idx[i] + 1]; }
    const double after = kp_mean_dist(sw, pk);
    if (after < dist) {
      dist = after;
      for (int k = 0; k < 18; ++k) ck[k] = sw[k];
    }
  }
  int nouf = st.nouf[t];
  if (dist < p.add_thr) {
    nouf = 0;
    for (int k = 0; k < 18; ++k) ck[k] = (1.0 - p.kp_speed) * pk[k] + p.kp_speed * ck[k];
  } else if (nouf > p.nouf_thresh) {
    // keypoints not updated for too long: take the new ones
  } else {
    for (int k = 0; k < 18; ++k) ck[k] = pk[k];
    nouf += 1;
  }
  st.nouf[t] = nouf;
  for (int k = 0; k < 18; ++k) st.kp[18 * (size_t)t + k] = ck[k];
}

__global__ __launch_bounds__(kLanes) void track_step_kernel(TrackArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int D = a.D, T = a.T;
  const TrackParams p = a.p;
  const LdsPlan l = lds_plan(D, T);
  double* u = reinterpret_cast<double*>(smem + l.off_u);
  double* v = reinterpret_cast<double*>(smem + l.off_v);
  double* minv = reinterpret_cast<double*>(smem + l.off_minv);
  float* cost = reinterpret_cast<float*>(smem + l.off_cost);
  int* pm = reinterpret_cast<int*>(smem + l.off_p);          // pm[j]: row (1-based) matched to column j; column 0 is virtual
  int* way = reinterpret_cast<int*>(smem + l.off_way);
  int* used = reinterpret_cast<int*>(smem + l.off_used);
  int* act = reinterpret_cast<int*>(smem + l.off_act);
  int* assign = reinterpret_cast<int*>(smem + l.off_assign);
  int* dbox = reinterpret_cast<int*>(smem + l.off_dbox);
  int* slot = reinterpret_cast<int*>(smem + l.off_slot);
  int* newid = reinterpret_cast<int*>(smem + l.off_newid);
  int* sh = reinterpret_cast<int*>(smem + l.off_sh);
  const StateView st = state_view(a.state + (size_t)s * a.state_stride, T);
  const unsigned long long lt = (1ull << lane) - 1ull;

  int nd = a.counts ? a.counts[s] : D;
  nd = min(max(nd, 0), D);
  const int time = st.hdr[H_TIME];
  int nt = min(max(st.hdr[H_NUM], 0), T);
  int last_id = st.hdr[H_LAST_ID], dropped = st.hdr[H_DROPPED], cleared = st.hdr[H_CLEARED];
  int head = min(max(st.hdr[H_RING_HEAD], 0), T - 1), cnt = min(max(st.hdr[H_RING_COUNT], 0), T);
  const int* dets = a.dets + (size_t)s * D * 4;
  const float* kps = a.kps + (size_t)s * D * 18;

  // ---- detections -> LDS; active tracks in list order (_continue_tracks, :194-197) --------------------------------
  for (int i = lane; i < nd * 4; i += kLanes) dbox[i] = dets[i];
  for (int i = lane; i < nd; i += kLanes) assign[i] = -1;
  int na = 0;
  for (int base = 0; base < nt; base += kLanes) {
    const int t = base + lane;
    const bool on = t < nt && st.end[t] >= time - p.continue_thresh;
    const unsigned long long m = __ballot(on);
    if (on) act[na + __popcll(m & lt)] = t;
    na += __popcll(m);
  }
  __syncthreads();

  if (nd > 0 && na > 0) {
    // ---- cost matrix [nd][na] (_compute_detections_assignment_cost, :234-243) --------------------------------------
    for (int e = lane; e < nd * na; e += kLanes) {
      const int i = e / na, j = e - i * na;
      cost[e] = (float)(0.5 * (1.0 - box_giou(dbox + 4 * i, st.box + 4 * act[j])));
    }
    // ---- minimum-cost assignment: shortest augmenting paths with potentials; rows = the shorter side ---------------
    const bool tr = nd > na;
    const int n = tr ? na : nd, m = tr ? nd : na;
    for (int j = lane; j <= m; j += kLanes) { pm[j] = 0; v[j] = 0.0; }
    for (int i = lane; i <= n; i += kLanes) u[i] = 0.0;
    __syncthreads();
    bool ok = true;
    for (int i = 1; i <= n && ok; ++i) {
      for (int j = lane; j <= m; j += kLanes) { minv[j] = INFINITY; used[j] = 0; }
      if (lane == 0) pm[0] = i;
      __syncthreads();
      int j0 = 0;
      do {
        if (lane == 0) used[j0] = 1;
        __syncthreads();
        const int i0 = pm[j0];
        const double ui0 = u[i0];
        double best = INFINITY;
        int bestj = INT_MAX;
        for (int j = 1 + lane; j <= m; j += kLanes) {      // the arg-min over the free columns, spread over the lanes
          if (used[j]) continue;
          const float c = tr ? cost[(j - 1) * na + (i0 - 1)] : cost[(i0 - 1) * na + (j - 1)];
          const double cur = (double)c - ui0 - v[j];
          if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
          if (minv[j] < best) { best = minv[j]; bestj = j; }
        }
        for (int o = 32; o > 0; o >>= 1) {                 // lowest column among equals
          const double ob = __shfl_xor(best, o, kLanes);
          const int oj = __shfl_xor(bestj, o, kLanes);
          if (ob < best || (ob == best && oj < bestj)) { best = ob; bestj = oj; }
        }
        if (bestj > m) { ok = false; break; }              // (no finite free column: cannot happen with finite costs)
        __syncthreads();
        for (int j = lane; j <= m; j += kLanes) {
          if (used[j]) { u[pm[j]] += best; v[j] -= best; }
          else minv[j] -= best;
        }
        j0 = bestj;
        __syncthreads();
      } while (pm[j0] != 0);
      if (ok && lane == 0) {
        do {
          const int j1 = way[j0];
          pm[j0] = pm[j1];
          j0 = j1;
        } while (j0);
      }
      __syncthreads();
    }
    // ---- gating (:204-208) -----------------------------------------------------------------------------------------
    for (int j = 1 + lane; j <= m && ok; j += kLanes) {
      if (!pm[j]) continue;
      const int det = tr ? j - 1 : pm[j] - 1, col = tr ? pm[j] - 1 : j - 1;
      if (cost[det * na + col] < (float)p.match_thr && box_iou(st.box + 4 * act[col], dbox + 4 * det) > p.iou_thr) assign[det] = col;
    }
    __syncthreads();
    // ---- Track.add_detection, one lane per matched detection (the tracks are distinct) ------------------------------
    for (int i = lane; i < nd; i += kLanes) {
      if (assign[i] < 0) continue;
      double nk[18];
      for (int k = 0; k < 18; ++k) nk[k] = (double)kps[(size_t)i * 18 + k];
      add_detection(st, act[assign[i]], dbox + 4 * i, nk, time, p);
    }
  }
  __syncthreads();

  // ---- _create_new_tracks (:245-260): slots and ids in detection order, then the copies in parallel -----------------
  if (lane == 0) {
    int n = nt;
    for (int i = 0; i < nd; ++i) {
      slot[i] = -1;
      if (assign[i] >= 0) continue;
      if (n >= T) { ++dropped; continue; }
      if (cnt > 0) {
        newid[i] = st.ring[head];
        head = head + 1 == T ? 0 : head + 1;
        --cnt;
      } else {
        newid[i] = last_id++;
      }
      slot[i] = n++;
    }
    sh[0] = n; sh[1] = head; sh[2] = cnt; sh[3] = last_id; sh[4] = dropped;
  }
  __syncthreads();
  nt = sh[0]; head = sh[1]; cnt = sh[2]; last_id = sh[3]; dropped = sh[4];
  for (int i = lane; i < nd; i += kLanes) {
    const int t = slot[i];
    if (t < 0) continue;
    st.id[t] = newid[i];
    st.end[t] = time;
    st.len[t] = 1;
    st.nouf[t] = 0;
    for (int c = 0; c < 4; ++c) st.box[4 * t + c] = dbox[4 * i + c];
    for (int k = 0; k < 18; ++k) st.kp[18 * (size_t)t + k] = (double)kps[(size_t)i * 18 + k];
  }
  __syncthreads();

  // ---- _clear_old_tracks (:219-232) as a stable compaction, 64 tracks at a time, and get_tracked_objects (:176-185) ---
  // a chunk is read into registers before any of it is written; its destinations are at or before its own positions
  int w = 0, oc = 0;
  int* ob = a.out_boxes + (size_t)s * T * 4;
  double* okp = a.out_kp + (size_t)s * T * 18;
  int* oi = a.out_ids + (size_t)s * T;
  for (int base = 0; base < nt; base += kLanes) {
    const int t = base + lane;
    const bool valid = t < nt;
    int id = 0, end = 0, len = 0, nouf = 0, bx[4] = {0, 0, 0, 0};
    double kp[18];
    if (valid) {
      id = st.id[t]; end = st.end[t]; len = st.len[t]; nouf = st.nouf[t];
      for (int c = 0; c < 4; ++c) bx[c] = st.box[4 * t + c];
      for (int k = 0; k < 18; ++k) kp[k] = st.kp[18 * (size_t)t + k];
    }
    const bool old = valid && end < time - p.clear_thresh;
    const bool rel = valid && !old && end < time - p.continue_thresh && len < p.time_window;
    const bool keep = valid && !old && !rel;
    const bool sel = keep && end == time;                      // touched by this frame: what get_tracked_objects returns
    const unsigned long long mk = __ballot(keep), mr = __ballot(rel), mo = __ballot(old), ms = __ballot(sel);
    if (rel) st.ring[(head + cnt + __popcll(mr & lt)) % T] = id;
    cnt += __popcll(mr);
    cleared += __popcll(mo);
    __syncthreads();
    if (keep) {
      const int d = w + __popcll(mk & lt);
      if (d != t) {
        st.id[d] = id; st.end[d] = end; st.len[d] = len; st.nouf[d] = nouf;
        for (int c = 0; c < 4; ++c) st.box[4 * d + c] = bx[c];
        for (int k = 0; k < 18; ++k) st.kp[18 * (size_t)d + k] = kp[k];
      }
    }
    if (sel) {
      const int o = oc + __popcll(ms & lt);
      oi[o] = len > p.time_window ? id : -1;
      for (int c = 0; c < 4; ++c) ob[4 * o + c] = bx[c];
      for (int k = 0; k < 18; ++k) okp[18 * (size_t)o + k] = kp[k];
    }
    w += __popcll(mk);
    oc += __popcll(ms);
    __syncthreads();
  }
  if (lane == 0) {
    st.hdr[H_TIME] = time + 1;
    st.hdr[H_NUM] = w;
    st.hdr[H_LAST_ID] = last_id;
    st.hdr[H_DROPPED] = dropped;
    st.hdr[H_CLEARED] = cleared;
    st.hdr[H_RING_HEAD] = head;
    st.hdr[H_RING_COUNT] = cnt;
    a.out_count[s] = oc;
    int* sc = a.out_scalars + 4 * (size_t)s;
    sc[0] = w; sc[1] = last_id; sc[2] = time + 1; sc[3] = dropped;
  }
}

}  // namespace

// include/t3d.h
extern "C" int t3d_track_state_bytes(int max_tracks) {
  if (max_tracks < 1 || max_tracks > (1 << 20)) return T3D_ERR_ARG;
  return (int)state_bytes(max_tracks);
}

extern "C" int t3d_track_lds_bytes(int max_dets, int max_tracks) {
  if (max_dets < 0 || max_tracks < 1) return T3D_ERR_ARG;
  if (lds_bytes_ll(max_dets, max_tracks) > INT_MAX) return INT_MAX;
  return lds_plan(max_dets, max_tracks).total;
}

extern "C" int t3d_track_step(void* state, const int* dets, const float* kps, const int* counts, int S, int max_dets,
                              int max_tracks, int time_window, int continue_time_thresh, int track_clear_thresh,
                              double match_threshold, double track_detection_iou_thresh, int interpolate_time_thresh,
                              double detection_filter_speed, double keypoints_filter_speed, double add_treshold,
                              int no_updated_frames_treshold, int align_kp, int* out_count, int* out_boxes, double* out_kp,
                              int* out_ids, int* out_scalars, void* stream) {
  (void)interpolate_time_thresh;      // stored by IOUTracker.__init__ (:156-157), read nowhere
  if (!state || !out_count || !out_boxes || !out_kp || !out_ids || !out_scalars) return T3D_ERR_ARG;
  if (S < 1 || max_dets < 0 || max_tracks < 1 || max_tracks > (1 << 20)) return T3D_ERR_ARG;
  if (max_dets > 0 && (!dets || !kps)) return T3D_ERR_ARG;
  if (time_window < 1 || continue_time_thresh < 1 || track_clear_thresh < 1 || no_updated_frames_treshold < 0) return T3D_ERR_ARG;
  if (lds_bytes_ll(max_dets, max_tracks) > kMaxLds) return T3D_ERR_UNSUPPORTED;
  const int lds = lds_plan(max_dets, max_tracks).total;
  if (lds > kMaxLds) return T3D_ERR_UNSUPPORTED;
  TrackArgs a{};
  a.state = static_cast<unsigned char*>(state);
  a.state_stride = state_bytes(max_tracks);
  a.dets = dets; a.kps = kps; a.counts = counts;
  a.D = max_dets; a.T = max_tracks;
  a.p = TrackParams{time_window, continue_time_thresh, track_clear_thresh, no_updated_frames_treshold, align_kp != 0,
                    match_threshold, track_detection_iou_thresh, detection_filter_speed, keypoints_filter_speed, add_treshold};
  a.out_count = out_count; a.out_boxes = out_boxes; a.out_kp = out_kp; a.out_ids = out_ids; a.out_scalars = out_scalars;
  if (lds > 64 * 1024) (void)t3d_max_lds((const void*)track_step_kernel, lds);
  T3D_LAUNCH(track_step_kernel, dim3(S), dim3(kLanes), lds, reinterpret_cast<hipStream_t>(stream), a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
