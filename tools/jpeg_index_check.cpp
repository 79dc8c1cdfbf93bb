// Host check of the JPEG indexer and of the code one device lane runs, meant to be built with the sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_index_check.cpp -o jpeg_index_check
//   ./jpeg_index_check DIR [--dump]
//
// DIR holds files (tests/test_jpeg_host.py writes its truncation and mutation corpus with T3D_JPEG_CORPUS=DIR).  Every file is
// copied into a heap block of exactly its size, so a read past `bytes` is a sanitizer report, and goes through
// t3d_jpeg_index_impl with segs = NULL and with a table of exactly nseg entries for several seg_mcus.  A file the indexer
// accepts is then decoded with the lane code of csrc/jpeg_decode.h -- the functions the kernels call, one "lane" after the
// other -- into buffers of exactly the sizes t3d_jpeg_decode_u8 is given; all seg_mcus must give the same pixels.
// Every accepted file is also decoded rectangle by rectangle (the whole image, 1 x 1 at the corners and the centre, the last row,
// the last column, interior rectangles on and off MCU and chroma-parity boundaries) through the lane code of
// t3d_jpeg_decode_roi_u8 -- roi_geom, roi_lane_segment, the same decode_segment with RECT set, idct_block on the compact
// workspace, colour_run_roi -- with only the planned byte span and the needed run of segments copied into heap blocks of exactly
// their sizes; each must equal the full decode's slice, and every needed segment must come up exactly once.
// --dump writes them to FILE.rgb (h * w * 3 bytes).  Exit status 0: every call returned T3D_OK, T3D_ERR_ARG or
// T3D_ERR_UNSUPPORTED, every accepted table lies inside its scan and every accepted file decoded with status 0.
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../3d-object-detection.pytorch_amd/csrc/jpeg_decode.h"

namespace L = t3d_jpeg_lane;

// what the kernels set up around the lane calls: the four Huffman tables (DC 0, DC 1, AC 0, AC 1), each component's selectors
// into them, the quantisation tables widened to int
struct Tables {
  t3d_jpeg_huff tab[4];
  int dci[3], aci[3], quant[192];
  explicit Tables(const t3d_jpeg_info& info) {
    for (int t = 0; t < 2; ++t) {
      t3d_jpeg_build_huff(info.dc_bits[t], info.dc_vals[t], 16, &tab[t]);
      t3d_jpeg_build_huff(info.ac_bits[t], info.ac_vals[t], 256, &tab[2 + t]);
    }
    for (int c = 0; c < 3; ++c) {
      dci[c] = c < info.ncomp ? info.comp_dc[c] : 0, aci[c] = 2 + (c < info.ncomp ? info.comp_ac[c] : 0);
      for (int k = 0; k < 64; ++k) quant[64 * c + k] = info.quant[c][k];
    }
  }
};

static bool decode(const unsigned char* data, long long bytes, const t3d_jpeg_info& info, const t3d_jpeg_seg* segs,
                   std::vector<unsigned char>* rgb) {
  t3d_jpeg_item it = {0, bytes, 0, 0, 0, 0};
  const long long nblocks = (long long)info.mcus_x * info.mcus_y * t3d_jpeg_mcu_blocks(info.sampling);
  const long long out_bytes = (long long)info.h * info.w * 3;
  unsigned char* out = (unsigned char*)malloc(out_bytes);
  void* work = aligned_alloc(16, (size_t)((nblocks * 192 + 15) / 16 * 16));
  memset(work, 0, (size_t)nblocks * 128);
  const L::Geom g = L::geom(data, bytes, &info, segs, info.nseg, it, out, out_bytes, work, nblocks);
  bool ok = g.ok;
  if (ok) {
    const Tables T(info);
    const L::Roi r = L::whole(g);
    for (int s = 0; s < g.nseg; ++s) ok = L::decode_segment<false>(r, T.tab, T.dci, T.aci, s) && ok;
    for (long long b = 0; b < g.nblocks; ++b) L::idct_block(g, T.quant, b);
    const long long nrun = ((long long)g.h * g.w + 3) / 4;
    for (long long t = 0; t < nrun; ++t) L::colour_run(g, t, (t & 1) != 0);      // (both store paths)
    rgb->assign(out, out + out_bytes);
  }
  free(work);
  free(out);
  return ok;
}

// the rectangle [x0, x1) x [y0, y1) of an accepted file against `full`, the full decode -> findings
static long long n_rects = 0;
static int decode_rect(const unsigned char* data, const t3d_jpeg_info& info, const t3d_jpeg_seg* segs,
                       const std::vector<unsigned char>& full, int x0, int y0, int x1, int y1, const char* name) {
  const L::McuRect mr = L::roi_mcus(info.sampling, info.h, info.w, x0, y0, x1, y1);
  const int S = info.seg_mcus, X = info.mcus_x;
  const int s_lo = (mr.my0 * X + mr.mx0) / S, s_hi = ((mr.my1 - 1) * X + mr.mx1 - 1) / S;
  const long long first = segs[s_lo].byte;
  long long end = s_hi + 1 < info.nseg ? (long long)segs[s_hi + 1].byte + 8 : info.scan_bytes;
  if (end > info.scan_bytes) end = info.scan_bytes;
  const long long nspan = end - first, nseg = s_hi - s_lo + 1;
  unsigned char* span = (unsigned char*)malloc(nspan > 0 ? nspan : 1);      // exactly the span: a read outside it is a report
  memcpy(span, data + info.scan_offset + first, (size_t)nspan);
  t3d_jpeg_seg* part = (t3d_jpeg_seg*)malloc(sizeof(t3d_jpeg_seg) * (size_t)nseg);
  memcpy(part, segs + s_lo, sizeof(t3d_jpeg_seg) * (size_t)nseg);
  const long long nblocks = (long long)(mr.mx1 - mr.mx0) * (mr.my1 - mr.my0) * t3d_jpeg_mcu_blocks(info.sampling);
  const long long out_bytes = (long long)(y1 - y0) * (x1 - x0) * 3;
  unsigned char* out = (unsigned char*)malloc(out_bytes + 1) + 1;            // (an odd address: the byte stores, and dwords where a run aligns)
  void* work = aligned_alloc(16, (size_t)((nblocks * 192 + 15) / 16 * 16));
  memset(work, 0, (size_t)nblocks * 128);
  t3d_jpeg_item it = {0, nspan, 0, 0, 0, first};
  const int rect[12] = {x0, y0, x1, y1, mr.mx0, mr.my0, mr.mx1, mr.my1, s_lo, (int)nseg, 0, 0};
  const L::Roi r = L::roi_geom(span, nspan, &info, part, nseg, it, rect, out, out_bytes, work, nblocks);
  int bad = 0;
  ++n_rects;
  if (!r.g.ok) {
    printf("%s: rectangle %d %d %d %d refused\n", name, x0, y0, x1, y1), ++bad;
  } else {
    const Tables T(info);
    std::vector<int> seen((size_t)nseg, 0);
    bool ok = true;
    const long long lanes = (long long)(r.my1 - r.my0) * r.per_row;
    for (long long t = 0; t < lanes; ++t) {
      const int s = L::roi_lane_segment(r, t);
      if (s < 0) continue;
      if (s < s_lo || s > s_hi || seen[s - s_lo]++) printf("%s: segment %d outside the needed run, or twice\n", name, s), ++bad;
      else ok = L::decode_segment<true>(r, T.tab, T.dci, T.aci, s) && ok;
    }
    for (int my = mr.my0; my < mr.my1; ++my)                                  // every segment that owns an MCU of the rectangle came up
      for (int mx = mr.mx0; mx < mr.mx1; ++mx)
        if (!seen[(my * X + mx) / S - s_lo]) printf("%s: segment of MCU %d %d not decoded\n", name, my, mx), ++bad, seen[(my * X + mx) / S - s_lo] = 1;
    if (!ok) printf("%s: rectangle %d %d %d %d did not decode\n", name, x0, y0, x1, y1), ++bad;
    for (long long b = 0; b < r.g.nblocks; ++b) L::idct_block(r.g, T.quant, b);
    const long long nrun = (long long)(y1 - y0) * ((x1 - x0 + 3) >> 2);
    for (long long t = 0; t < nrun; ++t) L::colour_run_roi(r, t);
    for (int y = y0; y < y1 && !bad; ++y)
      if (memcmp(out + (long long)(y - y0) * (x1 - x0) * 3, full.data() + ((long long)y * info.w + x0) * 3, (size_t)(x1 - x0) * 3))
        printf("%s: rectangle %d %d %d %d differs from the full decode in row %d\n", name, x0, y0, x1, y1, y), ++bad;
  }
  free(work);
  free(out - 1);
  free(part);
  free(span);
  return bad;
}

static int decode_rects(const unsigned char* data, const t3d_jpeg_info& info, const t3d_jpeg_seg* segs,
                        const std::vector<unsigned char>& full, const char* name) {
  const int h = info.h, w = info.w;
  int bad = decode_rect(data, info, segs, full, 0, 0, w, h, name);
  const int pts[5][2] = {{0, 0}, {w - 1, 0}, {0, h - 1}, {w - 1, h - 1}, {w / 2, h / 2}};
  for (int k = 0; k < 5; ++k) bad += decode_rect(data, info, segs, full, pts[k][0], pts[k][1], pts[k][0] + 1, pts[k][1] + 1, name);
  bad += decode_rect(data, info, segs, full, 0, h - 1, w, h, name);
  bad += decode_rect(data, info, segs, full, w - 1, 0, w, h, name);
  const int starts[6] = {7, 8, 9, 15, 16, 17};
  for (int k = 0; k < 6; ++k) {
    const int a = starts[k];
    if (a < w) bad += decode_rect(data, info, segs, full, a, 0, std::min(w, a + 5), h, name);
    if (a < h) bad += decode_rect(data, info, segs, full, 0, a, w, std::min(h, a + 5), name);
    if (a < w && a < h) bad += decode_rect(data, info, segs, full, a, a, std::min(w, a + 11), std::min(h, a + 10), name);
  }
  return bad;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s DIR [--dump]\n", argv[0]);
    return 2;
  }
  const bool dump = argc > 2 && std::string(argv[2]) == "--dump";
  std::vector<std::string> names;
  DIR* d = opendir(argv[1]);
  if (!d) {
    perror(argv[1]);
    return 2;
  }
  while (dirent* e = readdir(d)) {
    const std::string n = e->d_name;
    if (n != "." && n != ".." && (n.size() < 4 || n.substr(n.size() - 4) != ".rgb")) names.push_back(n);
  }
  closedir(d);
  std::sort(names.begin(), names.end());
  long long n_ok = 0, n_arg = 0, n_uns = 0, n_bad = 0;
  for (const std::string& name : names) {
    const std::string path = std::string(argv[1]) + "/" + name;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) continue;
    fseek(f, 0, SEEK_END);
    const long long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char* data = (unsigned char*)malloc(bytes > 0 ? bytes : 1);
    if (bytes > 0 && fread(data, 1, bytes, f) != (size_t)bytes) return 2;
    fclose(f);
    std::vector<unsigned char> first;
    int rc0 = 1;
    const int seg_choices[4] = {1, 3, 8, 1 << 30};
    for (int k = 0; k < 4; ++k) {
      t3d_jpeg_info info;
      const int rc = t3d_jpeg_index_impl(data, bytes, seg_choices[k], &info, nullptr, 0);
      if (rc != T3D_OK && rc != T3D_ERR_ARG && rc != T3D_ERR_UNSUPPORTED) {
        printf("%s: return code %d\n", name.c_str(), rc), ++n_bad;
        break;
      }
      if (k == 0) rc0 = rc, (rc == T3D_OK ? n_ok : rc == T3D_ERR_ARG ? n_arg : n_uns) += 1;
      if (rc != rc0) printf("%s: seg_mcus %d returns %d, seg_mcus 1 returned %d\n", name.c_str(), seg_choices[k], rc, rc0), ++n_bad;
      if (rc != T3D_OK) break;
      t3d_jpeg_seg* segs = (t3d_jpeg_seg*)malloc(sizeof(t3d_jpeg_seg) * (size_t)info.nseg);
      t3d_jpeg_info again;
      if (t3d_jpeg_index_impl(data, bytes, seg_choices[k], &again, segs, info.nseg) != T3D_OK || memcmp(&info, &again, sizeof(info)))
        printf("%s: the call with a table disagrees with the call without\n", name.c_str()), ++n_bad;
      if (info.nseg > 1 && t3d_jpeg_index_impl(data, bytes, seg_choices[k], &again, segs, info.nseg - 1) != T3D_ERR_ARG)
        printf("%s: a table one entry short was accepted\n", name.c_str()), ++n_bad;
      if (info.scan_offset < 0 || info.scan_bytes < 0 || info.scan_offset + info.scan_bytes > bytes)
        printf("%s: the scan leaves the file\n", name.c_str()), ++n_bad;
      for (int s = 0; s < info.nseg; ++s)
        if (segs[s].byte >= info.scan_bytes || segs[s].bit > 7 || segs[s].mcu != (long long)s * seg_choices[k])
          printf("%s: segment %d lies outside the scan\n", name.c_str(), s), ++n_bad;
      std::vector<unsigned char> rgb;
      if (!decode(data, bytes, info, segs, &rgb)) printf("%s: seg_mcus %d did not decode\n", name.c_str(), seg_choices[k]), ++n_bad;
      if (k == 0) first = rgb;
      else if (rgb != first) printf("%s: seg_mcus %d gives other pixels than seg_mcus 1\n", name.c_str(), seg_choices[k]), ++n_bad;
      if (rgb.size() == (size_t)info.h * info.w * 3) n_bad += decode_rects(data, info, segs, rgb, name.c_str());
      free(segs);
    }
    if (dump && rc0 == T3D_OK) {
      FILE* o = fopen((path + ".rgb").c_str(), "wb");
      if (o) fwrite(first.data(), 1, first.size(), o), fclose(o);
    }
    free(data);
  }
  printf("%lld files: %lld accepted and decoded, %lld malformed, %lld unsupported, %lld rectangles compared, %lld findings\n",
         (long long)names.size(), n_ok, n_arg, n_uns, n_rects, n_bad);
  return n_bad ? 1 : 0;
}
