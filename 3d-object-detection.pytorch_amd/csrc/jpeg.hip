// Baseline JPEG frames decoded on the device from the host's MCU index: t3d_jpeg_index (host only, csrc/jpeg_index.h) and
// t3d_jpeg_decode_u8.  include/t3d.h states the arithmetic (libjpeg's JDCT_ISLOW + fancy upsampling, all integer); the numpy
// restatement tests/jpeg_ref.py and Pillow on libjpeg-turbo agree with it bit for bit.
//
// One call is two memsets (coefficients, status) and three kernels, whatever the batch:
//   entropy   one lane per SEGMENT (seg_mcus consecutive MCUs), one wave per workgroup, the workgroups of grid row y share
//             image y: its four Huffman tables are expanded into LDS once (a 9-bit first-level lookup + the canonical slow
//             path), every lane then runs the serial decode of its own segment from the indexed bit position with a 64-bit
//             window, four stream bytes per refill.  Lanes diverge (that is the nature of the format); what they share is the
//             table in LDS.  Non-zero quantised coefficients go to zeroed int16 blocks in natural order.
//   idct      one lane per 8x8 block: dequantise, the two islow passes in registers, one uint8 plane per component.
//   colour    four consecutive pixels per lane: chroma upsampling (4:2:0) and YCbCr -> RGB, three dword stores where the image
//             is dword aligned (a 1440 x 1920 frame is), bytes where it is not.
// t3d_jpeg_decode_roi_u8 is the same five enqueues for a pixel RECTANGLE of each file (the regression loader's crops): the
// entropy lanes are the segments that own an MCU of the rectangle's MCU rectangle, each once; coefficient and sample blocks exist
// for that MCU rectangle only, so the memset, the IDCT and the colour pass scale with the crop; the bytes may be the part of the
// scan those segments lie in.
// Both entry points decode ITEMS, windows of an image (csrc/jpeg_decode.h: the whole image, or a rectangle), with the same
// segment parser, IDCT and pixel arithmetic; here they share the argument list (JPEG_ARGS) and the argument checks
// (check_call).  Each kernel keeps its own lines around the lane calls, the table expansion of the two entropy kernels
// included: one body for both windows, and one function for the tables, change the kernels' code, and the whole-frame and
// the rectangle call were measured slower with them (finding 71).  As they stand the six kernels are the
// instructions they were before the parsers became one.  An entry point also keeps its grid -- a whole frame's from
// segments and blocks, a rectangle's from the planner's lanes and runs -- and its two memsets, which common.h's rule wants
// in front of its launches.
// Memory safety is in the code, not in the stream: the reader clamps every index to the image's scan and feeds zeros behind
// it, the block loop ends at coefficient 63, a lane stays inside its segment's blocks, and every per-image range is checked
// against the buffers before anything of that image is touched (status 2).
#include "common.h"
#include "jpeg_decode.h"

extern "C" int t3d_jpeg_index(const unsigned char* data, long long bytes, int seg_mcus, t3d_jpeg_info* info, t3d_jpeg_seg* segs,
                              long long seg_capacity) {
  return t3d_jpeg_index_impl(data, bytes, seg_mcus, info, segs, seg_capacity);
}

namespace {

namespace L = t3d_jpeg_lane;
static_assert(sizeof(t3d_jpeg_info) == 864 && sizeof(t3d_jpeg_seg) == 16 && sizeof(t3d_jpeg_item) == 48, "include/t3d.h");

// the buffers of a call, in the ABI's order; the rectangle kernels put `const int *__restrict__ rects,` into the slot behind items
#define JPEG_ARGS(...)                                                                                                         \
  const unsigned char *__restrict__ data, long long data_bytes, const t3d_jpeg_info *__restrict__ infos,                       \
      const t3d_jpeg_seg *__restrict__ segs, long long total_segs, const t3d_jpeg_item *__restrict__ items,                    \
      __VA_ARGS__ unsigned char *out, long long out_bytes, void *work, long long total_blocks
#define JPEG_RECTS const int *__restrict__ rects,
// item i of the call, checked: the whole image, or the rectangle rects[i] of it
#define JPEG_GEOM(i) L::geom(data, data_bytes, infos + (i), segs, total_segs, items[i], out, out_bytes, work, total_blocks)
#define JPEG_ROI(i) L::roi_geom(data, data_bytes, infos + (i), segs, total_segs, items[i], rects + 12 * (i), out, out_bytes, work, total_blocks)

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(JPEG_ARGS(), int* __restrict__ status) {
  __shared__ t3d_jpeg_huff tab[4];                      // DC 0, DC 1, AC 0, AC 1
  __shared__ int tab_ok[4];
  const int img = blockIdx.y;
  const L::Roi r = L::whole(JPEG_GEOM(img));            // (the one copy of the geometry here: a second one changes the code)
  const L::Geom& g = r.g;
  if (!g.ok) {                                          // (uniform in the workgroup)
    if (blockIdx.x == 0 && threadIdx.x == 0) status[img] = 2;
    return;
  }
  const t3d_jpeg_info* info = infos + img;
  if (threadIdx.x < 4) {
    const int t = threadIdx.x & 1;
    tab_ok[threadIdx.x] = threadIdx.x < 2 ? t3d_jpeg_build_huff(info->dc_bits[t], info->dc_vals[t], 16, &tab[threadIdx.x])
                                          : t3d_jpeg_build_huff(info->ac_bits[t], info->ac_vals[t], 256, &tab[threadIdx.x]);
  }
  __syncthreads();
  int dci[3], aci[3];
  bool tables = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    dci[c] = c < g.ncomp ? info->comp_dc[c] : 0;        // (0 or 1: L::geom checked them)
    aci[c] = 2 + (c < g.ncomp ? info->comp_ac[c] : 0);
    tables = tables && tab_ok[dci[c]] && tab_ok[aci[c]];
  }
  if (!tables) {
    if (blockIdx.x == 0 && threadIdx.x == 0) status[img] = 2;
    return;
  }
  for (int s = blockIdx.x * 64 + threadIdx.x; s < g.nseg; s += gridDim.x * 64)
    if (!L::decode_segment<false>(r, tab, dci, aci, s)) status[img] = 1;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(JPEG_ARGS()) {
  __shared__ int quant[3 * 64];
  const int img = blockIdx.y;
  const L::Geom g = JPEG_GEOM(img);
  if (!g.ok) return;
  if (threadIdx.x < 192) quant[threadIdx.x] = infos[img].quant[threadIdx.x >> 6][threadIdx.x & 63];
  __syncthreads();
  for (long long blk = blockIdx.x * 256ll + threadIdx.x; blk < g.nblocks; blk += gridDim.x * 256ll) L::idct_block(g, quant, blk);
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(JPEG_ARGS()) {
  const L::Geom g = JPEG_GEOM(blockIdx.y);
  if (!g.ok) return;
  const long long nrun = ((long long)g.h * g.w + 3) / 4;
  const bool aligned = (reinterpret_cast<uintptr_t>(g.out) & 3) == 0;        // (uniform in the workgroup)
  for (long long t = blockIdx.x * 256ll + threadIdx.x; t < nrun; t += gridDim.x * 256ll) L::colour_run(g, t, aligned);
}

// ---- a pixel rectangle per item: the grid is sized for the call's largest, so the workgroups a smaller one does not need leave first
__global__ __launch_bounds__(64) void jpeg_roi_entropy_kernel(JPEG_ARGS(JPEG_RECTS), int* __restrict__ status) {
  __shared__ t3d_jpeg_huff tab[4];                      // DC 0, DC 1, AC 0, AC 1
  __shared__ int tab_ok[4];
  const int img = blockIdx.y;
  const L::Roi r = JPEG_ROI(img);
  if (!r.g.ok) {                                        // (uniform in the workgroup)
    if (blockIdx.x == 0 && threadIdx.x == 0) status[img] = 2;
    return;
  }
  const long long lanes = (long long)(r.my1 - r.my0) * r.per_row;
  if (blockIdx.x * 64ll >= lanes) return;               // (uniform)
  const t3d_jpeg_info* info = infos + img;
  if (threadIdx.x < 4) {
    const int t = threadIdx.x & 1;
    tab_ok[threadIdx.x] = threadIdx.x < 2 ? t3d_jpeg_build_huff(info->dc_bits[t], info->dc_vals[t], 16, &tab[threadIdx.x])
                                          : t3d_jpeg_build_huff(info->ac_bits[t], info->ac_vals[t], 256, &tab[threadIdx.x]);
  }
  __syncthreads();
  int dci[3], aci[3];
  bool tables = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    dci[c] = c < r.g.ncomp ? info->comp_dc[c] : 0;      // (0 or 1: L::roi_geom checked them)
    aci[c] = 2 + (c < r.g.ncomp ? info->comp_ac[c] : 0);
    tables = tables && tab_ok[dci[c]] && tab_ok[aci[c]];
  }
  if (!tables) {
    if (threadIdx.x == 0) status[img] = 2;
    return;
  }
  for (long long t = blockIdx.x * 64ll + threadIdx.x; t < lanes; t += gridDim.x * 64ll) {
    const int s = L::roi_lane_segment(r, t);
    if (s >= 0 && !L::decode_segment<true>(r, tab, dci, aci, s)) status[img] = 1;
  }
}

__global__ __launch_bounds__(256) void jpeg_roi_idct_kernel(JPEG_ARGS(JPEG_RECTS)) {
  __shared__ int quant[3 * 64];
  const int img = blockIdx.y;
  const L::Roi r = JPEG_ROI(img);
  if (!r.g.ok || blockIdx.x * 256ll >= r.g.nblocks) return;
  if (threadIdx.x < 192) quant[threadIdx.x] = infos[img].quant[threadIdx.x >> 6][threadIdx.x & 63];
  __syncthreads();
  for (long long blk = blockIdx.x * 256ll + threadIdx.x; blk < r.g.nblocks; blk += gridDim.x * 256ll) L::idct_block(r.g, quant, blk);
}

__global__ __launch_bounds__(256) void jpeg_roi_colour_kernel(JPEG_ARGS(JPEG_RECTS)) {
  const L::Roi r = JPEG_ROI(blockIdx.y);
  if (!r.g.ok) return;
  const long long nrun = (long long)(r.y1 - r.y0) * ((r.x1 - r.x0 + 3) >> 2);
  for (long long t = blockIdx.x * 256ll + threadIdx.x; t < nrun; t += gridDim.x * 256ll) L::colour_run_roi(r, t);
}

// What both entry points check of their arguments (ptrs: every pointer is there; bounds: every grid bound is >= 1).
// -> T3D_ERR_ARG, or T3D_OK: for B == 0 nothing else was looked at and nothing is to be done
int check_call(int B, bool ptrs, long long data_bytes, long long total_segs, long long out_bytes, const void* work, long long work_bytes,
               long long total_blocks, bool bounds) {
  if (B < 0 || B > 65535) return T3D_ERR_ARG;
  if (B == 0) return T3D_OK;
  if (!ptrs || !bounds) return T3D_ERR_ARG;
  if (data_bytes <= 0 || total_segs <= 0 || out_bytes <= 0 || total_blocks <= 0 || total_blocks > (1ll << 40)) return T3D_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(work) & 15) || work_bytes < total_blocks * 192) return T3D_ERR_ARG;
  return T3D_OK;
}

}  // namespace

extern "C" int t3d_jpeg_decode_work_bytes(long long total_blocks, long long* bytes) {
  if (!bytes || total_blocks < 0 || total_blocks > (1ll << 40)) return T3D_ERR_ARG;
  *bytes = total_blocks * 192;
  return T3D_OK;
}

extern "C" int t3d_jpeg_decode_u8(const unsigned char* data, long long data_bytes, const t3d_jpeg_info* infos, const t3d_jpeg_seg* segs,
                                  long long total_segs, const t3d_jpeg_item* items, unsigned char* out, long long out_bytes, void* work,
                                  long long work_bytes, long long total_blocks, int* status, int B, int max_segs, int max_blocks,
                                  void* stream) {
  const int rc = check_call(B, data && infos && segs && items && out && work && status, data_bytes, total_segs, out_bytes, work, work_bytes,
                            total_blocks, max_segs >= 1 && max_blocks >= 1);
  if (rc != T3D_OK || B == 0) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(work, 0, (size_t)total_blocks * 128, st) != hipSuccess) return T3D_ERR_LAUNCH;
  if (hipMemsetAsync(status, 0, sizeof(int) * (size_t)B, st) != hipSuccess) return T3D_ERR_LAUNCH;
  const unsigned int gs = (unsigned int)min(max_segs / 64 + 1, 65535);
  T3D_LAUNCH(jpeg_entropy_kernel, dim3(gs, B), dim3(64), 0, st, data, data_bytes, infos, segs, total_segs, items, out, out_bytes, work,
             total_blocks, status);
  T3D_CHECK_LAUNCH();
  const unsigned int gb = (unsigned int)min(max_blocks / 256 + 1, 4096);
  T3D_LAUNCH(jpeg_idct_kernel, dim3(gb, B), dim3(256), 0, st, data, data_bytes, infos, segs, total_segs, items, out, out_bytes, work,
             total_blocks);
  T3D_CHECK_LAUNCH();
  const unsigned int gc = (unsigned int)min((max_blocks * 16ll + 255) / 256, 4096ll);      // a block is 64 samples = 16 runs of 4 pixels
  T3D_LAUNCH(jpeg_colour_kernel, dim3(gc, B), dim3(256), 0, st, data, data_bytes, infos, segs, total_segs, items, out, out_bytes, work,
             total_blocks);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

extern "C" int t3d_jpeg_decode_roi_u8(const unsigned char* data, long long data_bytes, const t3d_jpeg_info* infos, const t3d_jpeg_seg* segs,
                                      long long total_segs, const t3d_jpeg_item* items, const int* rects, unsigned char* out,
                                      long long out_bytes, void* work, long long work_bytes, long long total_blocks, int* status, int B,
                                      long long max_lanes, int max_blocks, long long max_runs, void* stream) {
  const int rc = check_call(B, data && infos && segs && items && rects && out && work && status, data_bytes, total_segs, out_bytes, work,
                            work_bytes, total_blocks, max_lanes >= 1 && max_blocks >= 1 && max_runs >= 1);
  if (rc != T3D_OK || B == 0) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(work, 0, (size_t)total_blocks * 128, st) != hipSuccess) return T3D_ERR_LAUNCH;
  if (hipMemsetAsync(status, 0, sizeof(int) * (size_t)B, st) != hipSuccess) return T3D_ERR_LAUNCH;
  const unsigned int gs = (unsigned int)min((max_lanes + 63) / 64, 65535ll);
  T3D_LAUNCH(jpeg_roi_entropy_kernel, dim3(gs, B), dim3(64), 0, st, data, data_bytes, infos, segs, total_segs, items, rects, out, out_bytes,
             work, total_blocks, status);
  T3D_CHECK_LAUNCH();
  const unsigned int gb = (unsigned int)min(max_blocks / 256 + 1, 4096);
  T3D_LAUNCH(jpeg_roi_idct_kernel, dim3(gb, B), dim3(256), 0, st, data, data_bytes, infos, segs, total_segs, items, rects, out, out_bytes,
             work, total_blocks);
  T3D_CHECK_LAUNCH();
  const unsigned int gc = (unsigned int)min((max_runs + 255) / 256, 4096ll);
  T3D_LAUNCH(jpeg_roi_colour_kernel, dim3(gc, B), dim3(256), 0, st, data, data_bytes, infos, segs, total_segs, items, rects, out, out_bytes,
             work, total_blocks);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
