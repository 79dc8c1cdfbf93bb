// cv::resize INTER_LINEAR on 8-bit data, the per-axis coefficients (shared by crop.hip and augment.hip).
//
//   source coordinate  fx = (float)((dx + 0.5) * (sw / ow) - 0.5),  sx = floor(fx),  fx -= sx
//   sx < 0 -> sx = 0, fx = 0;   sx >= sw-1 -> sx = sw-1, fx = 0      (columns);   rows are clipped to [0, sh-1] instead
//   11-bit fixed-point weights  a1 = rint(fx * 2048), a0 = rint((1 - fx) * 2048)   (round half to even)
//   horizontal  D = S[sx] * a0 + S[sx+1] * a1;   vertical  out = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2
// OpenCV is not a dependency: parity with cv2 itself is UNPINNED; oracle/crop_resize.py is the same restatement in numpy.
#pragma once
#include <hip/hip_runtime.h>

struct T3dLin { int i0, i1, w0, w1; };

// column rule (zero the fraction at the borders) or row rule (clip the two taps)
static __device__ __forceinline__ T3dLin lin_coef(int d, int ssize, int dsize, bool column) {
  const double scale = (double)ssize / (double)dsize;
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  T3dLin r;
  if (column) {
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= ssize - 1) { s = ssize - 1; f = 0.f; }
    r.i0 = s;
    r.i1 = min(s + 1, ssize - 1);
  } else {
    r.i0 = min(max(s, 0), ssize - 1);
    r.i1 = min(max(s + 1, 0), ssize - 1);
  }
  r.w0 = (int)rintf((1.f - f) * 2048.f);
  r.w1 = (int)rintf(f * 2048.f);
  return r;
}

// the vertical pass of one channel: two horizontal sums (11-bit weights each) -> uint8
static __device__ __forceinline__ int lin_vert(int d0, int d1, const T3dLin& cy) {
  const int v = (((cy.w0 * (d0 >> 4)) >> 16) + ((cy.w1 * (d1 >> 4)) >> 16) + 2) >> 2;
  return min(max(v, 0), 255);
}
