// t3d_detect_draw: the per-sample draws, MinIoURandomCrop's search, the box arithmetic and the t3d_det_sample records of one
// detection batch in ONE launch, on tables that live in device memory (torchdet3d/dataloaders/detection_arena.py); and
// t3d_detect_draw_host, the same arithmetic on the CPU (host only: no HIP call).  csrc/detect_draw.h is the arithmetic;
// include/t3d.h states the contract.
//
// The walk of one sample is serial -- every draw of the search depends on the one before -- and its length differs from
// sample to sample by orders of magnitude (a median of 15 to 313 draws, thousands at the far end).  So a sample gets a WAVE of
// its own and lane 0 walks: samples that share a wave would each wait for the longest of them and pay for every branch the
// others take, while B waves on 256 CUs run side by side at their own pace and the launch lasts as long as its longest search.
// The other 63 lanes leave at once; the boxes (at most 64) stay in the sample's own output rows, which the L1 holds.
// Contraction is off for the whole library (build.py) and, so that it does not depend on a flag, for this file by pragma: a fused
// multiply-add anywhere in the search changes a crop.
#pragma clang fp contract(off)
#include "common.h"
#include "detect_draw.h"

namespace {

namespace D = t3d_draw;
static_assert(sizeof(t3d_det_sample) == 80, "include/t3d.h");

__global__ __launch_bounds__(64) void detect_draw_kernel(D::Cfg cfg, D::Key key, const long long* __restrict__ frames, int B,
                                                         D::Tables tables, int G, t3d_det_sample* records, float* gt_boxes,
                                                         int* gt_labels, int* gt_counts, int* diag) {
  const int i = blockIdx.x;
  if (threadIdx.x != 0 || i >= B) return;
  D::sample(cfg, key, i, frames + 4ll * i, tables, G, records + i, gt_boxes + 4ll * G * i, gt_labels + (long long)G * i, gt_counts + i,
            diag + 2ll * i);
}

void pack(const double* cfg, const unsigned int* key, int n_key, D::Cfg* c, D::Key* k) {
  for (int j = 0; j < D::N_CFG; ++j) c->v[j] = cfg[j];
  for (int j = 0; j < D::MAX_KEY + 3; ++j) k->w[j] = j < n_key ? key[j] : 0u;
  k->n = n_key;
}

}  // namespace

extern "C" int t3d_detect_draw(const double* cfg, int n_cfg, const unsigned int* key, int n_key, const long long* frames, int B,
                               const float* boxes, const int* labels, const long long* box_start, long long n_images,
                               long long n_boxes, int G, void* records, float* gt_boxes, int* gt_labels, int* gt_counts, int* diag,
                               void* stream) {
  const int rc = D::check(cfg, n_cfg, key, n_key, frames, B, boxes, labels, box_start, n_images, n_boxes, G, records, gt_boxes, gt_labels,
                          gt_counts, diag);
  if (rc != T3D_OK || B == 0) return rc;
  D::Cfg c;
  D::Key k;
  pack(cfg, key, n_key, &c, &k);
  const D::Tables t = {boxes, labels, box_start, n_images, n_boxes};
  T3D_LAUNCH(detect_draw_kernel, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), c, k, frames, B, t, G,
             static_cast<t3d_det_sample*>(records), gt_boxes, gt_labels, gt_counts, diag);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

extern "C" int t3d_detect_draw_host(const double* cfg, int n_cfg, const unsigned int* key, int n_key, const long long* frames, int B,
                                    const float* boxes, const int* labels, const long long* box_start, long long n_images,
                                    long long n_boxes, int G, void* records, float* gt_boxes, int* gt_labels, int* gt_counts, int* diag,
                                    void* stream) {
  (void)stream;
  const int rc = D::check(cfg, n_cfg, key, n_key, frames, B, boxes, labels, box_start, n_images, n_boxes, G, records, gt_boxes, gt_labels,
                          gt_counts, diag);
  if (rc != T3D_OK) return rc;
  D::Cfg c;
  D::Key k;
  pack(cfg, key, n_key, &c, &k);
  const D::Tables t = {boxes, labels, box_start, n_images, n_boxes};
  for (int i = 0; i < B; ++i)
    D::sample(c, k, i, frames + 4ll * i, t, G, static_cast<t3d_det_sample*>(records) + i, gt_boxes + 4ll * G * i, gt_labels + (long long)G * i,
              gt_counts + i, diag + 2ll * i);
  return T3D_OK;
}
