// The draws, the box arithmetic and the kernel record of ONE sample of a detection batch: what DetectionAugmentPipeline.draw,
// .boxes and .records (torchdet3d/dataloaders/detection.py) do on the host, restated operation by operation so that the results
// are theirs bit for bit (include/t3d.h next to t3d_detect_draw states the contract).  No HIP include: csrc/detect_draw.hip
// runs `sample` in a kernel, one sample a wave, and on the CPU (t3d_detect_draw_host), where the CPU suite holds it to numpy.
//
// The random numbers are numpy's: SeedSequence (pool of 4 words, the published hash-mix constants, generate_state) seeds
// PCG64 (the 128-bit LCG, XSL-RR output), and random() is (next64 >> 11) * 2^-53.
// Every floating-point operation is rounded on its own: the file that includes this is compiled with contraction off.
#ifndef T3D_DETECT_DRAW_H_
#define T3D_DETECT_DRAW_H_

#include "../../include/t3d.h"

#ifdef __HIPCC__
#define T3D_DRAW_FN __host__ __device__ __forceinline__
#else
#define T3D_DRAW_FN inline
#endif

namespace t3d_draw {

typedef unsigned int u32;
typedef unsigned long long u64;
typedef unsigned __int128 u128;

// ---- the compiled pipeline: cfg[] of the entry point, by position --------------------------------------------------------------
enum { C_PHOTO = 0, C_DELTA, C_CON_LO, C_CON_HI, C_SAT_LO, C_SAT_HI, C_HUE, C_P_ROT, C_EXP_LO, C_EXP_HI, C_EXP_P, C_CROP, C_MIN_SIZE,
       C_CMP_F32, C_N_MODES, C_MODES, MAX_MODES = 16, C_P_FLIP = C_MODES + MAX_MODES, C_OH, C_OW, N_CFG };
enum { MAX_KEY = 16, DRAWS = 18, MAX_G = 64, TAG_LO = 0x0A7E11F2u, TAG_HI = 0x5D3Cu };      // detection.py: _CROP_TAG, two words
struct Cfg { double v[N_CFG]; };
struct Key { u32 w[MAX_KEY + 3]; int n; };      // (room for the crop search's three further words)
static_assert(N_CFG == 34, "include/t3d.h states the layout of cfg");

// ---- numpy.random.SeedSequence -----------------------------------------------------------------------------------------------
T3D_DRAW_FN u32 hashmix(u32 value, u32& hash_const, u32 mult) {
  value ^= hash_const;
  hash_const *= mult;
  value *= hash_const;
  return value ^ (value >> 16);
}
T3D_DRAW_FN u32 mix(u32 x, u32 y) {
  const u32 r = 0xca01f9ddu * x - 0x4973f715u * y;
  return r ^ (r >> 16);
}

struct Pcg64 {
  u128 state, inc;
  long long drawn;
};
T3D_DRAW_FN u128 pcg_mult() { return ((u128)2549297995355413924ull << 64) | 4865540595714422341ull; }
T3D_DRAW_FN void pcg_step(Pcg64& g) { g.state = g.state * pcg_mult() + g.inc; }

// default_rng(words): key.w are the uint32 words SeedSequence makes of its integers
T3D_DRAW_FN Pcg64 seeded(const Key& key) {
  const int n = key.n;
  u32 pool[4], hc = 0x43b0d7e5u;
  for (int i = 0; i < 4; ++i) pool[i] = hashmix(i < n ? key.w[i] : 0u, hc, 0x931e8875u);
  for (int s = 0; s < 4; ++s)
    for (int d = 0; d < 4; ++d)
      if (s != d) pool[d] = mix(pool[d], hashmix(pool[s], hc, 0x931e8875u));
  for (int s = 4; s < n; ++s)
    for (int d = 0; d < 4; ++d) pool[d] = mix(pool[d], hashmix(key.w[s], hc, 0x931e8875u));
  u32 st[8];
  hc = 0x8b51f9ddu;
  for (int i = 0; i < 8; ++i) {                     // generate_state(4, uint64): eight words, the low word of each first
    u32 v = pool[i & 3] ^ hc;
    hc *= 0x58f38dedu;
    v *= hc;
    st[i] = v ^ (v >> 16);
  }
  const u64 s0 = st[0] | ((u64)st[1] << 32), s1 = st[2] | ((u64)st[3] << 32), i0 = st[4] | ((u64)st[5] << 32),
            i1 = st[6] | ((u64)st[7] << 32);
  Pcg64 g;
  g.drawn = 0;
  g.state = 0;
  g.inc = ((((u128)i0 << 64) | i1) << 1) | 1;       // pcg64_srandom_r
  pcg_step(g);
  g.state += ((u128)s0 << 64) | s1;
  pcg_step(g);
  return g;
}

// skip `delta` outputs: the LCG's jump-ahead (pcg_advance_lcg_128)
T3D_DRAW_FN void advance(Pcg64& g, u64 delta) {
  u128 acc_mult = 1, acc_plus = 0, cur_mult = pcg_mult(), cur_plus = g.inc;
  while (delta > 0) {
    if (delta & 1) {
      acc_mult *= cur_mult;
      acc_plus = acc_plus * cur_mult + cur_plus;
    }
    cur_plus = (cur_mult + 1) * cur_plus;
    cur_mult *= cur_mult;
    delta >>= 1;
  }
  g.state = acc_mult * g.state + acc_plus;
}

T3D_DRAW_FN double uniform(Pcg64& g) {
  pcg_step(g);
  const u64 hi = (u64)(g.state >> 64), lo = (u64)g.state, x = hi ^ lo;
  const unsigned rot = (unsigned)(g.state >> 122);
  const u64 r = (x >> rot) | (x << ((64 - rot) & 63));
  ++g.drawn;
  return (double)(r >> 11) * (1.0 / 9007199254740992.0);
}

// ---- one sample ---------------------------------------------------------------------------------------------------------------
struct Tables {
  const float* boxes;            // [n_boxes, 4]
  const int* labels;             // [n_boxes]
  const long long* box_start;    // [n_images + 1]
  long long n_images, n_boxes;
};

T3D_DRAW_FN float lin32(double lo, double hi, double u) { return (float)(lo + (hi - lo) * u); }
T3D_DRAW_FN float fmax32(float a, float b) { return a > b ? a : b; }       // (np.maximum / np.minimum of finite numbers)
T3D_DRAW_FN float fmin32(float a, float b) { return a < b ? a : b; }

T3D_DRAW_FN void zero_sample(t3d_det_sample* rec, float* gb, int* gl, int* count, int* diag, int G) {
  unsigned char* r = reinterpret_cast<unsigned char*>(rec);
  for (int k = 0; k < (int)sizeof(t3d_det_sample); ++k) r[k] = 0;
  for (int k = 0; k < 4 * G; ++k) gb[k] = 0.f;
  for (int k = 0; k < G; ++k) gl[k] = 0;
  *count = 0;
  diag[0] = -1;
  diag[1] = 0;
}

// Sample i of the batch.  frame = (offset, h, w, dataset index); gb [G, 4], gl [G], count, diag [2] are the sample's own output
// rows -- gb and gl also hold the boxes while the search runs, so nothing else is written and nothing is allocated.
T3D_DRAW_FN void sample(const Cfg& cfg, const Key& key, int i, const long long* frame, const Tables& t, int G, t3d_det_sample* rec,
                        float* gb, int* gl, int* count, int* diag) {
  zero_sample(rec, gb, gl, count, diag, G);
  const long long off = frame[0], fh = frame[1], fw = frame[2], idx = frame[3];
  if (fh < 1 || fw < 1 || fh > (1 << 24) || fw > (1 << 24) || off < 0 || idx < 0 || idx >= t.n_images) return;
  const long long b0 = t.box_start[idx], b1 = t.box_start[idx + 1];
  if (b0 < 0 || b1 < b0 || b1 > t.n_boxes || b1 - b0 > G) return;
  int n = (int)(b1 - b0);
  const double* c = cfg.v;
  const int oh = (int)c[C_OH], ow = (int)c[C_OW];

  // draw(): this sample's 18 numbers of default_rng(key).random((B, 18))
  Pcg64 g = seeded(key);
  advance(g, (u64)DRAWS * (u64)i);
  double u[DRAWS];
  for (int k = 0; k < DRAWS; ++k) u[k] = uniform(g);
  const bool on = c[C_PHOTO] != 0;
  const bool bright = on && u[0] < .5, contrast = on && u[2] < .5, first = u[4] < .5, sat_on = on && u[5] < .5, hue_on = on && u[7] < .5;
  const bool turn = u[11] < c[C_P_ROT], expand = u[13] < c[C_EXP_P], flip = u[17] < c[C_P_FLIP];
  const int turns = turn ? (u[12] < .5 ? 1 : 3) : 0;
  int p = 0;
  if (on && u[9] < .5) {
    const long long q = (long long)(u[10] * 6);
    p = q > 5 ? 5 : (int)q;
  }

  // boxes(): the quarter turn, the paste
  int h = (int)fh, w = (int)fw;
  for (int k = 0; k < n; ++k) {
    const float* s = t.boxes + 4 * (b0 + k);
    float x0 = s[0], y0 = s[1], x1 = s[2], y1 = s[3];
    if (turns == 1) {                  // np.rot90(frame, 1): x' = y, y' = w - x
      const float a = (float)w - x1, b = (float)w - x0;
      x0 = y0, x1 = y1, y0 = a, y1 = b;
    } else if (turns == 3) {           // np.rot90(frame, 3): x' = h - y, y' = x
      const float a = (float)h - y1, b = (float)h - y0;
      y0 = x0, y1 = x1, x0 = a, x1 = b;
    }
    gb[4 * k] = x0, gb[4 * k + 1] = y0, gb[4 * k + 2] = x1, gb[4 * k + 3] = y1;
    gl[k] = t.labels[b0 + k];
  }
  if (turns) {
    const int s = h;
    h = w, w = s;
  }
  int left = 0, top = 0;
  if (expand) {
    const double r = c[C_EXP_LO] + (c[C_EXP_HI] - c[C_EXP_LO]) * u[14];
    const int H = (int)((double)h * r), W = (int)((double)w * r);
    left = (int)(u[15] * (double)(W - w)), top = (int)(u[16] * (double)(H - h));
    for (int k = 0; k < n; ++k) {
      gb[4 * k] += (float)left, gb[4 * k + 1] += (float)top, gb[4 * k + 2] += (float)left, gb[4 * k + 3] += (float)top;
    }
    h = H, w = W;
  }

  // MinIoURandomCrop's rejection search, from the sample's own generator keyed (*key, _CROP_TAG, i)
  int px0 = 0, py0 = 0, px1 = w, py1 = h, mode_at = -1;
  bool cropped = false;
  u64 keep = ~0ull;                                                     // bit k: box k stays (n <= 64)
  if (c[C_CROP] != 0) {
    Key ck = key;
    ck.w[key.n] = TAG_LO, ck.w[key.n + 1] = TAG_HI, ck.w[key.n + 2] = (u32)i;
    ck.n = key.n + 3;
    Pcg64 cg = seeded(ck);
    const int n_modes = (int)c[C_N_MODES];
    const double lo = c[C_MIN_SIZE];
    const bool cmp32 = c[C_CMP_F32] != 0;
    for (;;) {
      const long long q = (long long)(uniform(cg) * (double)n_modes);
      mode_at = q >= n_modes ? n_modes - 1 : (int)q;
      const double mode = c[C_MODES + mode_at];
      if (mode == 1) break;
      for (int tries = 0; tries < 50; ++tries) {
        const double new_w = lo * (double)w + ((double)w - lo * (double)w) * uniform(cg);
        const double new_h = lo * (double)h + ((double)h - lo * (double)h) * uniform(cg);
        if (new_h / new_w < 0.5 || new_h / new_w > 2) continue;
        const double l = uniform(cg) * ((double)w - new_w);
        const double tp = uniform(cg) * ((double)h - new_h);
        const long long q0 = (long long)l, q1 = (long long)tp, q2 = (long long)(l + new_w), q3 = (long long)(tp + new_h);
        if (q2 == q0 || q3 == q1) continue;
        const float f0 = (float)q0, f1 = (float)q1, f2 = (float)q2, f3 = (float)q3;
        u64 mask = 0;
        if (n) {
          float lowest = 0.f;
          for (int k = 0; k < n; ++k) {
            const float x0 = gb[4 * k], y0 = gb[4 * k + 1], x1 = gb[4 * k + 2], y1 = gb[4 * k + 3];
            const float iw = fmax32(fmin32(x1, f2) - fmax32(x0, f0), 0.f), ih = fmax32(fmin32(y1, f3) - fmax32(y0, f1), 0.f);
            const float inter = iw * ih;
            const float area = (x1 - x0) * (y1 - y0), patch = (f2 - f0) * (f3 - f1);
            const float sum = area + patch;
            const float uni = sum - inter;
            const float iou = inter / fmax32(uni, 1e-6f);
            if (k == 0 || iou < lowest) lowest = iou;
            const float cx = (x0 + x1) / 2.f, cy = (y0 + y1) / 2.f;
            if (cx > f0 && cy > f1 && cx < f2 && cy < f3) mask |= 1ull << k;
          }
          // `iou.min() < mode`: a float32 against a Python float, by the installed numpy's promotion
          if (cmp32 ? lowest < (float)mode : (double)lowest < mode) continue;
          if (!mask) continue;
        }
        // The accepted patch leaves the loops through the sample's own record, in memory: carried out in four registers, the
        // gfx950 build kept cx1, cy1 and lost cx0, cy0 (the CPU build did not; tests/test_gpu_detect_draw.py is what sees it).
        rec->cx0 = (int)q0, rec->cy0 = (int)q1, rec->cx1 = (int)q2, rec->cy1 = (int)q3;
        keep = mask;
        cropped = true;
        break;
      }
      if (cropped) break;
    }
    diag[1] = cg.drawn > 0x7fffffffll ? 0x7fffffff : (int)cg.drawn;
    if (cropped) px0 = rec->cx0, py0 = rec->cy0, px1 = rec->cx1, py1 = rec->cy1;
  }
  diag[0] = mode_at;

  // the crop's mask, clip and shift; Resize and its clip; the flip
  const int cw = px1 - px0, ch = py1 - py0;
  const float sx = (float)((double)ow / (double)cw), sy = (float)((double)oh / (double)ch);
  const float f0 = (float)px0, f1 = (float)py0, f2 = (float)px1, f3 = (float)py1;
  int m = 0;
  for (int k = 0; k < n; ++k) {
    if (cropped && !((keep >> k) & 1)) continue;
    float x0 = gb[4 * k], y0 = gb[4 * k + 1], x1 = gb[4 * k + 2], y1 = gb[4 * k + 3];
    const int label = gl[k];
    if (cropped) {
      x0 = fmax32(x0, f0) - f0, y0 = fmax32(y0, f1) - f1, x1 = fmin32(x1, f2) - f0, y1 = fmin32(y1, f3) - f1;
    }
    x0 = fmin32(fmax32(x0 * sx, 0.f), (float)ow), y0 = fmin32(fmax32(y0 * sy, 0.f), (float)oh);
    x1 = fmin32(fmax32(x1 * sx, 0.f), (float)ow), y1 = fmin32(fmax32(y1 * sy, 0.f), (float)oh);
    if (flip) {
      const float a = (float)ow - x1, b = (float)ow - x0;
      x0 = a, x1 = b;
    }
    gb[4 * m] = x0, gb[4 * m + 1] = y0, gb[4 * m + 2] = x1, gb[4 * m + 3] = y1;      // (m <= k: in place)
    gl[m] = label;
    ++m;
  }
  for (int k = m; k < n; ++k) {
    gb[4 * k] = gb[4 * k + 1] = gb[4 * k + 2] = gb[4 * k + 3] = 0.f;
    gl[k] = 0;
  }
  *count = m;

  // records()
  rec->offset = off, rec->h = (int)fh, rec->w = (int)fw, rec->turns = turns, rec->left = left, rec->top = top;
  rec->cx0 = px0, rec->cy0 = py0, rec->cx1 = px1, rec->cy1 = py1;
  rec->flags = (flip ? T3D_DET_FLIP : 0) | (bright ? T3D_DET_BRIGHTNESS : 0) | (contrast ? T3D_DET_CONTRAST : 0) |
               (contrast && !first ? T3D_DET_CONTRAST_LAST : 0) | (on ? T3D_DET_HSV : 0) | (sat_on ? T3D_DET_SATURATION : 0) |
               (hue_on ? T3D_DET_HUE : 0);
  rec->delta = bright ? lin32(-c[C_DELTA], c[C_DELTA], u[1]) : 0.f;
  rec->alpha = contrast ? lin32(c[C_CON_LO], c[C_CON_HI], u[3]) : 1.f;
  rec->sat = sat_on ? lin32(c[C_SAT_LO], c[C_SAT_HI], u[6]) : 1.f;
  rec->hue = hue_on ? lin32(-c[C_HUE], c[C_HUE], u[8]) : 0.f;
  const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};     // itertools.permutations(range(3))
  rec->perm[0] = perms[p][0], rec->perm[1] = perms[p][1], rec->perm[2] = perms[p][2];
  rec->reserved = 0;
}

// What both entry points check of their arguments -> T3D_OK or T3D_ERR_ARG.  (With a crop, one mode must be 1: it is the mode
// that always returns, so the search ends with probability 1 whatever the boxes are.)
inline int check(const double* cfg, int n_cfg, const unsigned int* key, int n_key, const void* frames, int B, const void* boxes,
                 const void* labels, const void* box_start, long long n_images, long long n_boxes, int G, const void* records,
                 const void* gt_boxes, const void* gt_labels, const void* gt_counts, const void* diag) {
  if (!cfg || !key || !frames || !boxes || !labels || !box_start || !records || !gt_boxes || !gt_labels || !gt_counts || !diag)
    return T3D_ERR_ARG;
  if (n_cfg != N_CFG || n_key < 1 || n_key > MAX_KEY || B < 0 || B > 65535 || G < 1 || G > MAX_G || n_images < 0 || n_boxes < 0)
    return T3D_ERR_ARG;
  const int oh = (int)cfg[C_OH], ow = (int)cfg[C_OW], n_modes = (int)cfg[C_N_MODES];
  if (oh < 1 || ow < 1 || oh > (1 << 24) || ow > (1 << 24)) return T3D_ERR_ARG;
  if (!(cfg[C_EXP_LO] >= 1 && cfg[C_EXP_HI] >= cfg[C_EXP_LO] && cfg[C_EXP_HI] <= 64)) return T3D_ERR_ARG;
  if (cfg[C_CROP] != 0) {
    if (n_modes < 1 || n_modes > MAX_MODES || !(cfg[C_MIN_SIZE] > 0 && cfg[C_MIN_SIZE] <= 1)) return T3D_ERR_ARG;
    bool whole = false;
    for (int k = 0; k < n_modes; ++k) whole = whole || cfg[C_MODES + k] == 1;
    if (!whole) return T3D_ERR_ARG;
  }
  return T3D_OK;
}

}  // namespace t3d_draw

#endif /* T3D_DETECT_DRAW_H_ */
