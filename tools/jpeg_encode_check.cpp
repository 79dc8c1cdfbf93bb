// Host check of the JPEG encoder's table setup and of the code one device lane runs, meant to be built with the sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_encode_check.cpp -o jpeg_encode_check
//   ./jpeg_encode_check [DIR]
//
// Without DIR: t3d_jpeg_encode_setup's implementation (csrc/jpeg_encode.h: setup_impl, host code that fills a caller's struct)
// for every quality 1 .. 100, both samplings and the sizes 1x1, 8x8, 33x17, 1080x1920, 65535x1 and 1x65535 into a heap block
// of exactly the struct's size, so a write past it is a sanitizer report; the header must be 623 bytes, begin with SOI and end
// with the SOS segment; every refusal of the definition must be T3D_ERR_ARG and leave the struct alone.
// With DIR: every file H_W_Q_S_SEG_B_CAP_tag.rgb in it (B frames [H][W][3], quality Q, sampling S = 1 / 2, SEG MCUs a segment,
// CAP bytes a slot) goes through the lane code of csrc/jpeg_encode.h -- the functions the kernels call, one "lane" after the
// other, in the kernels' order -- with work and out in heap blocks of exactly the sizes t3d_jpeg_encode_u8 is given; the result
// rows and the slots are written to the same name with .out (tests/test_jpeg_encode_host.py compares them with the numpy
// restatement).  Exit status 0: all of that held.
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../3d-object-detection.pytorch_amd/csrc/jpeg_encode.h"

namespace E = t3d_jpeg_enc;

static int fail(const char* what, int a = 0, int b = 0, int c = 0) {
  fprintf(stderr, "jpeg_encode_check: %s (%d %d %d)\n", what, a, b, c);
  return 1;
}

static int check_setup() {
  const int sizes[6][2] = {{1, 1}, {8, 8}, {33, 17}, {1080, 1920}, {65535, 1}, {1, 65535}};
  for (int q = 1; q <= 100; ++q)
    for (int s = T3D_JPEG_444; s <= T3D_JPEG_420; ++s)
      for (const auto& hw : sizes) {
        t3d_jpeg_enc_tables* t = (t3d_jpeg_enc_tables*)malloc(sizeof(t3d_jpeg_enc_tables));
        const int rc = E::setup_impl(hw[0], hw[1], q, s, t);
        bool ok = rc == T3D_OK && t->header_bytes == E::kHeaderBytes && t->header[0] == 0xFF && t->header[1] == 0xD8 &&
                  t->header[E::kHeaderBytes - 14] == 0xFF && t->header[E::kHeaderBytes - 13] == 0xDA && t->header[E::kHeaderBytes] == 0;
        for (int c = 0; c < 2 && ok; ++c)
          for (int i = 0; i < 64; ++i) ok = ok && t->divisor[c][i] >= 8 && t->divisor[c][i] <= 2040 && t->divisor[c][i] % 8 == 0;
        int codes = 0;
        for (int k = 0; k < 4; ++k)
          for (int i = 0; i < 256; ++i) codes += t->huff[k][i] != 0;
        ok = ok && codes == 12 + 12 + 162 + 162;
        free(t);
        if (!ok) return fail("setup", hw[0], hw[1], q);
      }
  const int bad[8][4] = {{0, 8, 90, T3D_JPEG_420},     {8, 0, 90, T3D_JPEG_420},  {65536, 8, 90, T3D_JPEG_420}, {8, 65536, 90, T3D_JPEG_444},
                         {8, 8, 0, T3D_JPEG_420},      {8, 8, 101, T3D_JPEG_444}, {8, 8, 90, T3D_JPEG_GRAY},    {8, 8, 90, 3}};
  for (const auto& a : bad) {
    t3d_jpeg_enc_tables t;
    memset(&t, 0x5A, sizeof(t));
    if (E::setup_impl(a[0], a[1], a[2], a[3], &t) != T3D_ERR_ARG || t.h != 0x5A5A5A5A || t.header[0] != 0x5A) return fail("refusal", a[0], a[1], a[2]);
  }
  if (E::setup_impl(8, 8, 90, T3D_JPEG_420, nullptr) != T3D_ERR_ARG) return fail("refusal of NULL");
  return 0;
}

// t3d_jpeg_encode_u8 on the host: the kernels' work, lane by lane, in their order
static int encode(const unsigned char* frames, int B, const t3d_jpeg_enc_tables& t, int seg_mcus, long long cap, unsigned char* out,
                  t3d_jpeg_enc_result* results) {
  E::Geo g;
  if (!E::geo_of(B, t.h, t.w, t.sampling, seg_mcus, cap, &g)) return fail("geo_of");
  void* work = aligned_alloc(16, (size_t)((g.total + 15) / 16 * 16));
  memset(work, 0xA5, (size_t)g.total);                 // (what the call does not zero itself is not zero)
  memset((unsigned char*)work + g.off_stream, 0, (size_t)B * g.ushare);
  for (int i = 0; i < B; ++i) {
    short* coef = E::coef_of(g, work, i);
    unsigned long long* seg = E::seg_of(g, work, i);
    unsigned int* stream = E::stream_of(g, work, i);
    unsigned int* ff = E::ff_of(g, work, i);
    for (int b = 0; b < g.blocks; ++b) E::transform_block(g, frames + (long long)i * t.h * t.w * 3, &t.divisor[0][0], coef, b);
    for (int s = 0; s < g.nseg; ++s) seg[s] = E::walk_segment<false>(g, coef, &t.huff[0][0], s, nullptr, 0, 0);
    unsigned long long run = 0;
    for (int s = 0; s <= g.nseg; ++s) {
      const unsigned long long v = s < g.nseg ? seg[s] : 0;
      seg[s] = run, run += v;
    }
    const long long ub = E::scan_bytes(g, seg[g.nseg]);
    unsigned int nff = 0;
    if (ub >= 0) {
      for (int s = g.nseg - 1; s >= 0; --s) E::walk_segment<true>(g, coef, &t.huff[0][0], s, stream, seg[s], seg[g.nseg]);      // (any order)
      const long long nch = (ub + E::kChunk - 1) / E::kChunk;
      for (long long c = 0; c < nch; ++c) {
        const unsigned int v = E::chunk_ff(stream, c);
        ff[c] = nff, nff += v;
      }
    }
    results[i] = E::frame_result(g, seg[g.nseg], nff);
    if (results[i].overflow) continue;
    unsigned char* o = out + (long long)i * cap;
    memcpy(o, t.header, E::kHeaderBytes);
    const long long nch = (ub + E::kChunk - 1) / E::kChunk;
    for (long long c = 0; c < nch; ++c) E::scatter_chunk(stream, c, ub, o + E::kHeaderBytes + c * E::kChunk + ff[c]);
    o[results[i].bytes - 2] = 0xFF, o[results[i].bytes - 1] = 0xD9;
  }
  free(work);
  return 0;
}

int main(int argc, char** argv) {
  if (check_setup()) return 1;
  if (argc < 2) {
    printf("jpeg_encode_check: setup ok\n");
    return 0;
  }
  const std::string dir = argv[1];
  DIR* d = opendir(dir.c_str());
  if (!d) return fail("cannot open the directory");
  std::vector<std::string> names;
  while (dirent* e = readdir(d)) {
    const std::string n = e->d_name;
    if (n.size() > 4 && n.substr(n.size() - 4) == ".rgb") names.push_back(n);
  }
  closedir(d);
  int done = 0;
  for (const std::string& n : names) {
    int h, w, q, s, seg, B;
    long long cap;
    if (sscanf(n.c_str(), "%d_%d_%d_%d_%d_%d_%lld_", &h, &w, &q, &s, &seg, &B, &cap) != 7) return fail("file name");
    t3d_jpeg_enc_tables t;
    if (E::setup_impl(h, w, q, s, &t) != T3D_OK || B < 1 || B > 64) return fail("file name values");
    const size_t fb = (size_t)B * h * w * 3;
    unsigned char* frames = (unsigned char*)malloc(fb);
    FILE* f = fopen((dir + "/" + n).c_str(), "rb");
    if (!f || fread(frames, 1, fb, f) != fb) return fail("short file");
    fclose(f);
    unsigned char* out = (unsigned char*)malloc((size_t)B * cap);
    memset(out, 0xEE, (size_t)B * cap);
    std::vector<t3d_jpeg_enc_result> res(B);
    if (encode(frames, B, t, seg, cap, out, res.data())) return 1;
    f = fopen((dir + "/" + n.substr(0, n.size() - 4) + ".out").c_str(), "wb");
    if (!f || fwrite(res.data(), 16, B, f) != (size_t)B || fwrite(out, 1, (size_t)B * cap, f) != (size_t)B * cap) return fail("cannot write");
    fclose(f);
    free(out);
    free(frames);
    ++done;
  }
  printf("jpeg_encode_check: setup ok, %d files encoded\n", done);
  return 0;
}
