// On-device 2-D based 3-D IoU (torchdet3d/evaluation/metrics.py:70-89): per sample, both keypoint sets are lifted to
// 3-D boxes (lift_2d, torchdet3d/utils/geometry.py:51-108) and the IoU of the two boxes is computed the way
// objectron.dataset.{box,iou} does it: box fit by least squares, intersection of the two
// FITTED boxes, volumes of the RAW vertex sets.  fp64 throughout, one 128-thread workgroup per sample:
//
//   wave w (0: predicted, 1: ground truth)
//     M^T M (12 x 12) of the 16 x 12 EPnP system, built entry-wise from the 8 corner keypoints          (:65-89)
//     cyclic Jacobi eigen-decomposition, matrix + eigenvectors in LDS, lanes = rows                     (:90-91, np.linalg.eigh)
//     eigenvector of the smallest eigenvalue -> 4 control points, z < 0 sign rule -> 9 vertices         (:92-105)
//   wave 0, after the barrier
//     fit (scale = mean edge length per axis; because the scaled unit box is symmetric about its centre the least-
//       squares system [X 1] S = V decouples exactly: R = (1 / 4 s_a) sum_v sign_va V_v, t = mean_v V_v)
//     both boxes expressed in box 1's frame: box 1 = axis-aligned cuboid, box 2 = parallelepiped
//     intersection volume by the divergence theorem over the 12 clipped face polygons (lane f clips face f with
//       Sutherland-Hodgman against the other box's 6 half-spaces, thickness eps = 1e-6 like the reference's clipper):
//       V = 1/3 sum_f dist_f * area_f -- equal to the convex-hull volume of the reference's intersection point set,
//       because that set is exactly the vertex set of this convex polytope.  A face of box 2 that lies ON a face of
//       box 1 with the same outward direction would be counted twice and is dropped.
//     IoU = V / (vol1 + vol2 - V); singular fits and empty / flat intersections give 0 (the reference's
//       LinAlgError / QhullError / no-points cases, metrics.py:82-86).
#include "box_geometry.h"

namespace {

struct Smem {
  double A[2][12 * LD];
  double V[2][12 * LD];
  double vert[2][9][3];
  double poly[12][2][MAXV][3];
};

__global__ __launch_bounds__(128) void iou3d_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                    int portrait, double fx, double fy, double cx, double cy,
                                                    double* __restrict__ iou, double* __restrict__ total,
                                                    double* __restrict__ lifted, const double* __restrict__ verts) {
  __shared__ Smem sm;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (verts) {               // boxes given directly as 9 x 3 vertex sets (t3d_box_iou3d)
    if (tid < 54) sm.vert[tid / 27][(tid % 27) / 3][tid % 3] = verts[(size_t)b * 54 + tid];
  } else {
    const float* kp = (wave == 0 ? pred : gt) + (size_t)b * 18;
    lift_wave<float>(kp, portrait, fx, fy, cx, cy, sm.A[wave], sm.V[wave], sm.vert[wave], lane);
  }
  __syncthreads();
  if (lifted && tid < 54) lifted[(size_t)b * 54 + tid] = sm.vert[tid / 27][(tid % 27) / 3][tid % 3];
  if (!iou || wave != 0) return;

  const double r = box_iou_wave(sm.vert[0], sm.vert[1], sm.poly, lane);
  if (lane == 0) {
    iou[b] = r;
    if (total) atomicAdd(total, r);
  }
}

}  // namespace

extern "C" int t3d_iou3d(const float* pred_kp, const float* gt_kp, int B, int portrait, const double* camera_ndc,
                         double* iou, double* total, double* lifted, void* stream) {
  if (!pred_kp || !gt_kp || B <= 0 || (!iou && !lifted)) return T3D_ERR_ARG;
  // NDC camera of geometry.py:29-37 applied to the default matrix (:16-19): fx = fy = 2, cx = cy = 0
  double fx = 2.0, fy = 2.0, cx = 0.0, cy = 0.0;
  if (camera_ndc) { fx = camera_ndc[0]; fy = camera_ndc[1]; cx = camera_ndc[2]; cy = camera_ndc[3]; }
  T3D_LAUNCH(iou3d_kernel, dim3(B), dim3(128), 0, reinterpret_cast<hipStream_t>(stream), pred_kp, gt_kp, portrait,
                     fx, fy, cx, cy, iou, total, lifted, nullptr);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

extern "C" int t3d_box_iou3d(const double* verts, int B, double* iou, double* total, void* stream) {
  if (!verts || !iou || B <= 0) return T3D_ERR_ARG;
  T3D_LAUNCH(iou3d_kernel, dim3(B), dim3(128), 0, reinterpret_cast<hipStream_t>(stream), nullptr, nullptr, 0, 2.0,
                     2.0, 0.0, 0.0, iou, total, nullptr, verts);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
