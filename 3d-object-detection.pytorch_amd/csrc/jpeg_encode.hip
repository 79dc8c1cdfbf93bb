// Baseline JPEG encode on the device: t3d_jpeg_encode_setup (host only), t3d_jpeg_encode_work_bytes, t3d_jpeg_encode_u8.
// include/t3d.h states the arithmetic (libjpeg-turbo's default compression path as Pillow drives it, all integer); the numpy
// restatement tests/jpeg_encode_ref.py and Pillow on libjpeg-turbo write the same files byte for byte.  csrc/jpeg_encode.h holds
// what one lane does; here are the kernels around the lane calls and the entry points.
//
// One call is one memset (the unstuffed streams) and seven kernels, whatever the batch; grid row y is frame y:
//   transform  a lane per 8x8 block: colour, edges, downsampling, FDCT, quantisation -> int16 blocks in scan order, zig-zag
//   count      a lane per SEGMENT (seg_mcus consecutive MCUs), one wave per workgroup, the four code tables in LDS: the exact
//              bit length of the segment's codes
//   seg scan   a workgroup per frame: the exclusive scan of the bit lengths, the total behind them
//   emit       the count's walk again, now writing: whole words stored, the words shared with a neighbour OR-ed in
//   ff count   a lane per 64-byte chunk of the unstuffed stream: its FF bytes
//   ff scan    a workgroup per frame: the exclusive scan of those, the frame's result row, and -- if the file fits -- its header
//              and EOI
//   scatter    a lane per chunk: its bytes to their place in the file, a 00 behind every FF
// A frame whose scan or file does not fit is decided per frame from the scanned totals (uniform in the frame): its emit,
// ff count and scatter lanes leave at once, so it writes nothing but its result row.
// Memory safety is in the code: every index comes from the Geo the host made of checked arguments and passes by value; the
// device copy of the tables only supplies divisors (0 is read as 1), code words (a length is masked to 5 bits) and header
// bytes, and the emit lanes check every word index against the frame's share.
#include "common.h"
#include "jpeg_encode.h"

extern "C" int t3d_jpeg_encode_setup(int h, int w, int quality, int sampling, t3d_jpeg_enc_tables* out) {
  return t3d_jpeg_enc::setup_impl(h, w, quality, sampling, out);
}

namespace {

namespace E = t3d_jpeg_enc;
static_assert(sizeof(t3d_jpeg_enc_tables) == 5040 && offsetof(t3d_jpeg_enc_tables, divisor) == 48 &&
                  offsetof(t3d_jpeg_enc_tables, huff) == 304 && offsetof(t3d_jpeg_enc_tables, header) == 4400 &&
                  sizeof(t3d_jpeg_enc_result) == 16,
              "include/t3d.h; torchdet3d/utils/jpeg_encode.py mirrors the layout");

__global__ __launch_bounds__(256) void jpeg_enc_transform_kernel(E::Geo g, const unsigned char* __restrict__ frames,
                                                                 const t3d_jpeg_enc_tables* __restrict__ tables, void* work) {
  __shared__ unsigned short divisor[128];
  if (threadIdx.x < 128) {
    const unsigned short d = tables->divisor[threadIdx.x >> 6][threadIdx.x & 63];
    divisor[threadIdx.x] = d ? d : 1;
  }
  __syncthreads();
  const int img = blockIdx.y;
  const unsigned char* frame = frames + (long long)img * g.h * g.w * 3;
  short* coef = E::coef_of(g, work, img);
  for (long long t = blockIdx.x * 256ll + threadIdx.x; t < g.blocks; t += gridDim.x * 256ll) E::transform_block(g, frame, divisor, coef, (int)t);
}

// the four code tables of the device copy -> LDS, lengths masked
__device__ __forceinline__ void load_codes(const t3d_jpeg_enc_tables* tables, unsigned int* huff) {
  for (int i = threadIdx.x; i < 1024; i += blockDim.x) huff[i] = tables->huff[i >> 8][i & 255] & 0x1FFFFFu;
  __syncthreads();
}

__global__ __launch_bounds__(64) void jpeg_enc_count_kernel(E::Geo g, const t3d_jpeg_enc_tables* __restrict__ tables, void* work) {
  __shared__ unsigned int huff[1024];
  load_codes(tables, huff);
  const int img = blockIdx.y;
  const short* coef = E::coef_of(g, work, img);
  unsigned long long* seg = E::seg_of(g, work, img);
  for (long long s = blockIdx.x * 64ll + threadIdx.x; s < g.nseg; s += gridDim.x * 64ll)
    seg[s] = E::walk_segment<false>(g, coef, huff, (int)s, nullptr, 0, 0);
}

// a[0 .. n) -> its exclusive prefix sums in place, -> the total; the whole workgroup (256 threads) calls it
template <class T> __device__ T block_scan(T* a, long long n, T* sh) {
  const int tid = threadIdx.x;
  const long long per = (n + 255) / 256, i0 = E::lo(tid * per, n), i1 = E::lo(i0 + per, n);
  T sum = 0;
  for (long long i = i0; i < i1; ++i) sum += a[i];
  sh[tid] = sum;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const T v = tid >= d ? sh[tid - d] : 0;
    __syncthreads();
    sh[tid] += v;
    __syncthreads();
  }
  T run = sh[tid] - sum;
  const T total = sh[255];
  for (long long i = i0; i < i1; ++i) {
    const T v = a[i];
    a[i] = run;
    run += v;
  }
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(256) void jpeg_enc_seg_scan_kernel(E::Geo g, void* work) {
  __shared__ unsigned long long sh[256];
  unsigned long long* seg = E::seg_of(g, work, blockIdx.x);
  const unsigned long long total = block_scan(seg, (long long)g.nseg, sh);
  if (threadIdx.x == 0) seg[g.nseg] = total;
}

__device__ __forceinline__ long long scan_bytes(const E::Geo& g, const unsigned long long* seg) { return E::scan_bytes(g, seg[g.nseg]); }

__global__ __launch_bounds__(64) void jpeg_enc_emit_kernel(E::Geo g, const t3d_jpeg_enc_tables* __restrict__ tables, void* work) {
  __shared__ unsigned int huff[1024];
  load_codes(tables, huff);
  const int img = blockIdx.y;
  const short* coef = E::coef_of(g, work, img);
  const unsigned long long* seg = E::seg_of(g, work, img);
  if (scan_bytes(g, seg) < 0) return;                   // (uniform in the frame)
  unsigned int* stream = E::stream_of(g, work, img);
  for (long long s = blockIdx.x * 64ll + threadIdx.x; s < g.nseg; s += gridDim.x * 64ll)
    E::walk_segment<true>(g, coef, huff, (int)s, stream, seg[s], seg[g.nseg]);
}

__global__ __launch_bounds__(256) void jpeg_enc_ff_count_kernel(E::Geo g, void* work) {
  const int img = blockIdx.y;
  const long long ub = scan_bytes(g, E::seg_of(g, work, img));
  if (ub < 0) return;
  const long long nch = (ub + E::kChunk - 1) / E::kChunk;              // <= g.nchunk
  const unsigned int* stream = E::stream_of(g, work, img);
  unsigned int* ff = E::ff_of(g, work, img);
  for (long long c = blockIdx.x * 256ll + threadIdx.x; c < nch; c += gridDim.x * 256ll) ff[c] = E::chunk_ff(stream, c);
}

__global__ __launch_bounds__(256) void jpeg_enc_ff_scan_kernel(E::Geo g, const t3d_jpeg_enc_tables* __restrict__ tables, void* work,
                                                               unsigned char* out, t3d_jpeg_enc_result* results) {
  __shared__ unsigned int sh[256];
  const int img = blockIdx.x;
  const unsigned long long* seg = E::seg_of(g, work, img);
  const long long ub = scan_bytes(g, seg);
  if (ub < 0) {                                          // (uniform)
    if (threadIdx.x == 0) results[img] = E::frame_result(g, seg[g.nseg], 0);
    return;
  }
  const unsigned int nff = block_scan(E::ff_of(g, work, img), (ub + E::kChunk - 1) / E::kChunk, sh);
  const t3d_jpeg_enc_result res = E::frame_result(g, seg[g.nseg], nff);
  if (threadIdx.x == 0) results[img] = res;
  if (res.overflow) return;
  const long long bytes = res.bytes;
  unsigned char* o = out + (long long)img * g.cap;
  for (int i = threadIdx.x; i < E::kHeaderBytes; i += 256) o[i] = tables->header[i];
  if (threadIdx.x < 2) o[bytes - 2 + threadIdx.x] = threadIdx.x ? 0xD9 : 0xFF;
}

__global__ __launch_bounds__(256) void jpeg_enc_scatter_kernel(E::Geo g, void* work, unsigned char* out,
                                                               const t3d_jpeg_enc_result* __restrict__ results) {
  const int img = blockIdx.y;
  const long long ub = scan_bytes(g, E::seg_of(g, work, img));
  if (ub < 0 || results[img].overflow) return;          // (uniform in the frame)
  const long long nch = (ub + E::kChunk - 1) / E::kChunk;
  const unsigned int* stream = E::stream_of(g, work, img);
  const unsigned int* ff = E::ff_of(g, work, img);
  unsigned char* o = out + (long long)img * g.cap + E::kHeaderBytes;
  // (the ff scan found header + ub + all FF bytes + 2 <= cap: chunk c ends at or below o + ub + all FF bytes)
  for (long long c = blockIdx.x * 256ll + threadIdx.x; c < nch; c += gridDim.x * 256ll) E::scatter_chunk(stream, c, ub, o + c * E::kChunk + ff[c]);
}

// the caller's host tables are ones setup fills for their own h, w, sampling
bool tables_ok(const t3d_jpeg_enc_tables* t) {
  E::Grid gr;
  if (!E::grid_of(t->h, t->w, t->sampling, &gr) || t->quality < 1 || t->quality > 100) return false;
  return t->mcus_x == gr.mcus_x && t->mcus_y == gr.mcus_y && t->mcu_blocks == gr.bpm && t->blocks == gr.blocks &&
         t->luma_rows == gr.luma_rows && t->luma_cols == gr.luma_cols && t->header_bytes == E::kHeaderBytes;
}

}  // namespace

extern "C" int t3d_jpeg_encode_work_bytes(int B, int h, int w, int sampling, int seg_mcus, long long cap_bytes, long long* bytes) {
  E::Geo g;
  if (!bytes || !E::geo_of(B, h, w, sampling, seg_mcus, cap_bytes, &g)) return T3D_ERR_ARG;
  *bytes = g.total;
  return T3D_OK;
}

extern "C" int t3d_jpeg_encode_u8(const unsigned char* frames, int B, const t3d_jpeg_enc_tables* tables,
                                  const t3d_jpeg_enc_tables* tables_dev, int seg_mcus, unsigned char* out, long long cap_bytes,
                                  t3d_jpeg_enc_result* results, void* work, long long work_bytes, void* stream) {
  if (B < 0 || B > 65535) return T3D_ERR_ARG;
  if (B == 0) return T3D_OK;
  if (!frames || !tables || !tables_dev || !out || !results || !work || !tables_ok(tables)) return T3D_ERR_ARG;
  E::Geo g;
  if (!E::geo_of(B, tables->h, tables->w, tables->sampling, seg_mcus, cap_bytes, &g)) return T3D_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(work) & 15) || (reinterpret_cast<uintptr_t>(out) & 15) || work_bytes < g.total) return T3D_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(reinterpret_cast<unsigned char*>(work) + g.off_stream, 0, (size_t)B * (size_t)g.ushare, st) != hipSuccess) return T3D_ERR_LAUNCH;
  const unsigned int gt = (unsigned int)min((g.blocks + 255ll) / 256, 65535ll * 16);
  T3D_LAUNCH(jpeg_enc_transform_kernel, dim3(gt, B), dim3(256), 0, st, g, frames, tables_dev, work);
  T3D_CHECK_LAUNCH();
  const unsigned int gs = (unsigned int)min((g.nseg + 63ll) / 64, 65535ll * 16);
  T3D_LAUNCH(jpeg_enc_count_kernel, dim3(gs, B), dim3(64), 0, st, g, tables_dev, work);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(jpeg_enc_seg_scan_kernel, dim3(B), dim3(256), 0, st, g, work);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(jpeg_enc_emit_kernel, dim3(gs, B), dim3(64), 0, st, g, tables_dev, work);
  T3D_CHECK_LAUNCH();
  const unsigned int gc = (unsigned int)min((g.nchunk + 255) / 256, 4096ll);
  T3D_LAUNCH(jpeg_enc_ff_count_kernel, dim3(gc, B), dim3(256), 0, st, g, work);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(jpeg_enc_ff_scan_kernel, dim3(B), dim3(256), 0, st, g, tables_dev, work, out, results);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(jpeg_enc_scatter_kernel, dim3(gc, B), dim3(256), 0, st, g, work, out, results);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
