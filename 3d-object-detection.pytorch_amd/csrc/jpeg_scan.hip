// The MCU index of baseline JPEG files built on the device: t3d_jpeg_header (host only, csrc/jpeg_index.h) and
// t3d_jpeg_index_device.  include/t3d.h states the method; csrc/jpeg_scan.h is what one lane does, and also compiles for the
// host (tools/jpeg_scan_check.cpp).  The rows are those of the host indexer t3d_jpeg_index, byte for byte.
//
// One call is FOUR kernels, whatever the batch, and no memset:
//   speculate   one lane per SUBSEQUENCE (sub_bytes raw bytes of the stuffed scan), the workgroups of grid row y share image y
//               and its four Huffman tables in LDS; every lane decodes from its first byte as if an MCU began there and stores
//               its exit state and counts.  Workgroup 0 of a row also sets the image's status (1 until proven indexed, or 2),
//               its scan_bytes (-1 until then) and its head record.
//   settle      ONE workgroup per image, looping over that image's lanes: rounds of take / decode again, each followed by a
//               workgroup barrier, until no lane took a new entry -- at most nsub rounds; then the exclusive scan of the MCU
//               starts and DC sums over the image's lanes.  No workgroup ever waits for another one.
//   emit        the speculate grid again: every lane decodes with its true entry, MCU number and predictors, writes its rows,
//               flags failed checks; the lane in front of which the last MCU ends checks the trailer.
//   finish      one thread per image: status 0 and the scan's length where nothing was flagged and the trailer was in order.
// Memory safety is in the code, not in the stream: see csrc/jpeg_scan.h (image, Reader, run).
#include "common.h"
#include "jpeg_scan.h"

extern "C" int t3d_jpeg_header(const unsigned char* data, long long bytes, int seg_mcus, t3d_jpeg_info* info) {
  return t3d_jpeg_header_impl(data, bytes, seg_mcus, info);
}

namespace {

namespace S = t3d_jpeg_scan;
constexpr int kLaneThreads = 256, kSettleThreads = 512;
constexpr int kSubMin = 4, kSubMax = 1 << 30;

#define SCAN_ARGS                                                                                                              \
  const unsigned char *__restrict__ data, long long data_bytes, t3d_jpeg_info *infos, t3d_jpeg_seg *segs, long long total_segs, \
      const t3d_jpeg_item *__restrict__ items, int sub, void *work, long long work_bytes, int B
#define SCAN_IMAGE(i) S::image(data, data_bytes, infos + (i), segs, total_segs, items[i], sub, work, work_bytes, B, i)

struct Tables {
  t3d_jpeg_huff tab[4];                                 // DC 0, DC 1, AC 0, AC 1
  int ok[4];
};

// the image's tables into LDS (a barrier: every thread of the workgroup calls it) -> the tables its components use are prefix codes
__device__ bool expand_tables(const t3d_jpeg_info* info, int ncomp, Tables* T, int dci[3], int aci[3]) {
  if (threadIdx.x < 4) {
    const int t = threadIdx.x & 1;
    T->ok[threadIdx.x] = threadIdx.x < 2 ? t3d_jpeg_build_huff(info->dc_bits[t], info->dc_vals[t], 16, &T->tab[threadIdx.x])
                                         : t3d_jpeg_build_huff(info->ac_bits[t], info->ac_vals[t], 256, &T->tab[threadIdx.x]);
  }
  __syncthreads();
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    dci[c] = c < ncomp ? info->comp_dc[c] : 0;          // (0 or 1: S::image checked them)
    aci[c] = 2 + (c < ncomp ? info->comp_ac[c] : 0);
    ok = ok && T->ok[dci[c]] && T->ok[aci[c]];
  }
  return ok;
}

__global__ __launch_bounds__(kLaneThreads) void jpeg_scan_speculate_kernel(SCAN_ARGS, int* __restrict__ status) {
  __shared__ Tables T;
  const int img = blockIdx.y;
  const S::Img g = SCAN_IMAGE(img);                     // (uniform in the workgroup)
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (first) infos[img].scan_bytes = -1;
  if (!g.ok) {
    if (first) status[img] = 2;
    return;
  }
  int dci[3], aci[3];
  const bool tables = expand_tables(infos + img, g.ncomp, &T, dci, aci);
  if (first) {
    status[img] = tables ? 1 : 2;
    if (tables) g.head->err = 0, g.head->rounds = 0, g.head->end = -1;
  }
  if (!tables) return;
  for (long long j = blockIdx.x * (long long)kLaneThreads + threadIdx.x; j < g.nsub; j += gridDim.x * (long long)kLaneThreads)
    S::decode_into(g, T.tab, dci, aci, j, sub, S::guess(g, j, sub));
}

__global__ __launch_bounds__(kSettleThreads) void jpeg_scan_settle_kernel(SCAN_ARGS) {
  __shared__ Tables T;
  __shared__ unsigned int part[kSettleThreads][4];
  const int img = blockIdx.x, tid = threadIdx.x;
  const S::Img g = SCAN_IMAGE(img);
  if (!g.ok) return;
  int dci[3], aci[3];
  if (!expand_tables(infos + img, g.ncomp, &T, dci, aci)) return;
  // rounds to the fixed point: round r leaves lanes 0 .. r with their true entries, so nsub rounds suffice whatever the data
  long long rounds = 0;
  for (; rounds < g.nsub; ++rounds) {
    int took = 0;
    for (long long j = 1 + tid; j < g.nsub; j += kSettleThreads) took |= S::take(g.recs, j) ? 1 : 0;
    if (!__syncthreads_or(took)) break;
    for (long long j = 1 + tid; j < g.nsub; j += kSettleThreads) S::again(g, T.tab, dci, aci, j, sub);
    __syncthreads();
  }
  if (tid == 0) g.head->rounds = (int)S::lo(rounds, 0x7FFFFFFFll);
  // count: the exclusive scan of (MCU starts, DC sums) over the lanes; thread t owns the lanes [t * per, (t + 1) * per)
  const long long per = (g.nsub + kSettleThreads - 1) / kSettleThreads;
  const long long j0 = S::lo(tid * per, g.nsub), j1 = S::lo(j0 + per, g.nsub);
  unsigned int sum[4] = {0u, 0u, 0u, 0u};
  for (long long j = j0; j < j1; ++j) {
    const S::Rec& rec = g.recs[j];
    sum[0] += rec.mcus, sum[1] += rec.dc[0], sum[2] += rec.dc[1], sum[3] += rec.dc[2];
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) part[tid][v] = sum[v];
  __syncthreads();
  if (tid < 4) {                                        // (512 additions a value)
    unsigned int run = 0;
    for (int t = 0; t < kSettleThreads; ++t) {
      const unsigned int x = part[t][tid];
      part[t][tid] = run;
      run += x;
    }
  }
  __syncthreads();
#pragma unroll
  for (int v = 0; v < 4; ++v) sum[v] = part[tid][v];
  for (long long j = j0; j < j1; ++j) {
    S::Rec& rec = g.recs[j];
    const unsigned int x[4] = {rec.mcus, rec.dc[0], rec.dc[1], rec.dc[2]};
    rec.mcus = sum[0], rec.dc[0] = sum[1], rec.dc[1] = sum[2], rec.dc[2] = sum[3];
#pragma unroll
    for (int v = 0; v < 4; ++v) sum[v] += x[v];
  }
}

__global__ __launch_bounds__(kLaneThreads) void jpeg_scan_emit_kernel(SCAN_ARGS) {
  __shared__ Tables T;
  const int img = blockIdx.y;
  const S::Img g = SCAN_IMAGE(img);
  if (!g.ok) return;
  int dci[3], aci[3];
  if (!expand_tables(infos + img, g.ncomp, &T, dci, aci)) return;
  for (long long j = blockIdx.x * (long long)kLaneThreads + threadIdx.x; j < g.nsub; j += gridDim.x * (long long)kLaneThreads)
    S::emit(g, T.tab, dci, aci, j, sub);
}

// (status 1: speculate found the record and the tables in order, so the image's head record is written and inside work)
__global__ __launch_bounds__(256) void jpeg_scan_finish_kernel(t3d_jpeg_info* infos, const void* work, int* __restrict__ status, int B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B || status[i] != 1) return;
  const S::Head h = reinterpret_cast<const S::Head*>(work)[i];
  if (h.err == 0 && h.end >= 0) {
    infos[i].scan_bytes = h.end;
    status[i] = 0;
  }
}

bool sub_ok(int sub_bytes) { return sub_bytes >= kSubMin && sub_bytes <= kSubMax; }

}  // namespace

extern "C" int t3d_jpeg_index_work_bytes(long long total_scan_bytes, int B, int sub_bytes, long long* bytes) {
  if (!bytes || total_scan_bytes < 0 || total_scan_bytes > (1ll << 48) || B < 0 || B > 65535 || !sub_ok(sub_bytes)) return T3D_ERR_ARG;
  // a head record an image, then ceil(n_i / sub_bytes) subsequence records an image: at most total / sub_bytes + B of them
  *bytes = (2ll * B + total_scan_bytes / sub_bytes) * 32;
  return T3D_OK;
}

extern "C" int t3d_jpeg_index_device(const unsigned char* data, long long data_bytes, t3d_jpeg_info* infos, t3d_jpeg_seg* segs,
                                     long long total_segs, const t3d_jpeg_item* items, int sub_bytes, void* work, long long work_bytes,
                                     int* status, int B, int max_subs, void* stream) {
  if (B < 0 || B > 65535) return T3D_ERR_ARG;
  if (B == 0) return T3D_OK;
  if (!data || !infos || !segs || !items || !work || !status) return T3D_ERR_ARG;
  if (!sub_ok(sub_bytes) || data_bytes <= 0 || total_segs <= 0 || max_subs < 1) return T3D_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(work) & 15) || work_bytes < 32ll * B) return T3D_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned int gx = (unsigned int)min((max_subs + kLaneThreads - 1) / kLaneThreads, 65535);
  T3D_LAUNCH(jpeg_scan_speculate_kernel, dim3(gx, B), dim3(kLaneThreads), 0, st, data, data_bytes, infos, segs, total_segs, items, sub_bytes,
             work, work_bytes, B, status);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(jpeg_scan_settle_kernel, dim3(B), dim3(kSettleThreads), 0, st, data, data_bytes, infos, segs, total_segs, items, sub_bytes, work,
             work_bytes, B);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(jpeg_scan_emit_kernel, dim3(gx, B), dim3(kLaneThreads), 0, st, data, data_bytes, infos, segs, total_segs, items, sub_bytes, work,
             work_bytes, B);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(jpeg_scan_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, st, infos, work, status, B);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
