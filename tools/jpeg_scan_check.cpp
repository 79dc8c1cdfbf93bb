// Host check of the device JPEG indexer's lane code (csrc/jpeg_scan.h) against the host indexer (csrc/jpeg_index.h), meant to
// be built with the sanitizers for the by-hand run and without them for the suite:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_scan_check.cpp -o jpeg_scan_check
//   ./jpeg_scan_check DIR SUB_BYTES [SUB_BYTES ...]
//
// DIR holds files (tests/jpeg_cases.py: write_files).  Every file is copied into a heap block of exactly its size, goes through
// t3d_jpeg_header_impl and -- where the markers are accepted -- through the passes of t3d_jpeg_index_device as the kernels run
// them, lanes in a loop: speculate, settle rounds (take, then decode again) to the fixed point, the exclusive scan, emit, finish;
// for seg_mcus 1, 2, 3 and one segment per image and every SUB_BYTES given, with a row table of exactly nseg entries and a work
// buffer of exactly t3d_jpeg_index_work_bytes' size.  Compared with t3d_jpeg_index_impl for every file: the header's return
// code, reason and info; accept / refuse; scan_bytes; every row, byte for byte.  Per file and SUB_BYTES the settle rounds used
// are printed.  Exit status 0: no finding.
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../3d-object-detection.pytorch_amd/csrc/jpeg_scan.h"

namespace S = t3d_jpeg_scan;

// t3d_jpeg_index_device for one image -> its status; *rounds: the settle rounds used
static int index_lanes(const unsigned char* data, long long bytes, t3d_jpeg_info* info, t3d_jpeg_seg* segs, int sub, long long* rounds) {
  const long long total_scan = bytes - info->scan_offset, work_bytes = (2 + total_scan / sub) * 32;      // (t3d_jpeg_index_work_bytes, B = 1)
  void* work = aligned_alloc(32, (size_t)work_bytes);
  memset(work, 0xA5, (size_t)work_bytes);
  const t3d_jpeg_item it = {0, bytes, 0, 0, 0, 0};
  const S::Img g = S::image(data, bytes, info, segs, info->nseg, it, sub, work, work_bytes, 1, 0);
  int status = 2;
  t3d_jpeg_huff tab[4];
  int dci[3], aci[3];
  bool tables = g.ok;
  for (int t = 0; t < 2 && g.ok; ++t) {
    const bool d = t3d_jpeg_build_huff(info->dc_bits[t], info->dc_vals[t], 16, &tab[t]);
    const bool a = t3d_jpeg_build_huff(info->ac_bits[t], info->ac_vals[t], 256, &tab[2 + t]);
    for (int c = 0; c < info->ncomp; ++c) tables = tables && (info->comp_dc[c] != t || d) && (info->comp_ac[c] != t || a);
  }
  info->scan_bytes = -1;
  if (tables) {
    for (int c = 0; c < 3; ++c) dci[c] = c < g.ncomp ? info->comp_dc[c] : 0, aci[c] = 2 + (c < g.ncomp ? info->comp_ac[c] : 0);
    status = 1;
    g.head->err = 0, g.head->rounds = 0, g.head->end = -1;
    for (long long j = 0; j < g.nsub; ++j) S::decode_into(g, tab, dci, aci, j, sub, S::guess(g, j, sub));      // speculate
    long long r = 0;
    for (; r < g.nsub; ++r) {                                                                                  // settle
      bool took = false;
      for (long long j = 1; j < g.nsub; ++j) took = S::take(g.recs, j) || took;
      if (!took) break;
      for (long long j = 1; j < g.nsub; ++j) S::again(g, tab, dci, aci, j, sub);
    }
    *rounds = r;
    unsigned int sum[4] = {0, 0, 0, 0};                                                                        // count
    for (long long j = 0; j < g.nsub; ++j) {
      S::Rec& rec = g.recs[j];
      const unsigned int x[4] = {rec.mcus, rec.dc[0], rec.dc[1], rec.dc[2]};
      rec.mcus = sum[0], rec.dc[0] = sum[1], rec.dc[1] = sum[2], rec.dc[2] = sum[3];
      for (int v = 0; v < 4; ++v) sum[v] += x[v];
    }
    for (long long j = g.nsub - 1; j >= 0; --j) S::emit(g, tab, dci, aci, j, sub);      // emit (any order: the lanes are independent)
    if (g.head->err == 0 && g.head->end >= 0) info->scan_bytes = g.head->end, status = 0;                      // finish
  }
  free(work);
  return status;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s DIR SUB_BYTES [SUB_BYTES ...]\n", argv[0]);
    return 2;
  }
  std::vector<int> subs;
  for (int k = 2; k < argc; ++k) subs.push_back(atoi(argv[k]));
  std::vector<std::string> names;
  DIR* d = opendir(argv[1]);
  if (!d) {
    perror(argv[1]);
    return 2;
  }
  while (dirent* e = readdir(d)) {
    const std::string n = e->d_name;
    if (n != "." && n != "..") names.push_back(n);
  }
  closedir(d);
  std::sort(names.begin(), names.end());
  long long n_ok = 0, n_refused = 0, n_header = 0, n_bad = 0, max_rounds = 0, n_runs = 0;
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
    const int seg_choices[4] = {1, 2, 3, 1 << 30};
    for (int k = 0; k < 4; ++k) {
      t3d_jpeg_info want, head;
      const int rc = t3d_jpeg_index_impl(data, bytes, seg_choices[k], &want, nullptr, 0);
      const int rh = t3d_jpeg_header_impl(data, bytes, seg_choices[k], &head);
      if (rh != T3D_OK) {                               // the markers refuse it: so does the indexer, with the same words
        if (k == 0) ++n_header;
        if (rh != rc || memcmp(&want, &head, sizeof(want)))
          printf("%s: the header returns %d (reason %d), the indexer %d (reason %d), or their infos differ\n", name.c_str(), rh, head.reason, rc,
                 want.reason), ++n_bad;
        continue;
      }
      if (head.scan_bytes != bytes - head.scan_offset) printf("%s: the header's clamp\n", name.c_str()), ++n_bad;
      std::vector<t3d_jpeg_seg> rows((size_t)(rc == T3D_OK ? want.nseg : 0));
      if (rc == T3D_OK && t3d_jpeg_index_impl(data, bytes, seg_choices[k], &want, rows.data(), want.nseg) != T3D_OK)
        printf("%s: the indexer refuses its own table\n", name.c_str()), ++n_bad;
      for (int sub : subs) {
        t3d_jpeg_info info = head;
        t3d_jpeg_seg* segs = (t3d_jpeg_seg*)malloc(sizeof(t3d_jpeg_seg) * (size_t)(info.nseg > 0 ? info.nseg : 1));      // exactly nseg rows
        memset(segs, 0xA5, sizeof(t3d_jpeg_seg) * (size_t)info.nseg);
        long long rounds = 0;
        const int status = index_lanes(data, bytes, &info, segs, sub, &rounds);
        ++n_runs;
        max_rounds = std::max(max_rounds, rounds);
        if (k == 0) printf("%s sub_bytes %d: status %d, %lld settle rounds, %lld lanes\n", name.c_str(), sub, status, rounds,
                           (bytes - info.scan_offset + sub - 1) / sub);
        if (k == 0 && sub == subs[0]) (status == 0 ? n_ok : n_refused) += 1;
        if (status == 2) printf("%s: sub_bytes %d: the lanes call the header's record inconsistent\n", name.c_str(), sub), ++n_bad;
        if ((status == 0) != (rc == T3D_OK)) {
          printf("%s: seg_mcus %d sub_bytes %d: the lanes give status %d, the indexer returns %d\n", name.c_str(), seg_choices[k], sub, status, rc), ++n_bad;
        } else if (status == 0) {
          if (memcmp(&info, &want, sizeof(info)))
            printf("%s: seg_mcus %d sub_bytes %d: scan_bytes %lld, the indexer's %lld (or another field differs)\n", name.c_str(), seg_choices[k],
                   sub, info.scan_bytes, want.scan_bytes), ++n_bad;
          for (int s = 0; s < want.nseg; ++s)
            if (memcmp(&segs[s], &rows[(size_t)s], sizeof(t3d_jpeg_seg))) {
              printf("%s: seg_mcus %d sub_bytes %d: row %d is (%u, %d, %d %d %d, mcu %d, %d), the indexer's (%u, %d, %d %d %d, mcu %d, %d)\n",
                     name.c_str(), seg_choices[k], sub, s, segs[s].byte, segs[s].bit, segs[s].pred[0], segs[s].pred[1], segs[s].pred[2],
                     segs[s].mcu, segs[s].reserved, rows[(size_t)s].byte, rows[(size_t)s].bit, rows[(size_t)s].pred[0], rows[(size_t)s].pred[1],
                     rows[(size_t)s].pred[2], rows[(size_t)s].mcu, rows[(size_t)s].reserved),
                  ++n_bad;
              break;
            }
        } else if (info.scan_bytes != -1) {
          printf("%s: a refused image keeps scan_bytes %lld\n", name.c_str(), info.scan_bytes), ++n_bad;
        }
        free(segs);
      }
    }
    free(data);
  }
  printf("%lld files: %lld accepted, %lld refused by the scan, %lld refused by the markers, %lld runs compared, most settle rounds %lld, "
         "%lld findings\n",
         (long long)names.size(), n_ok, n_refused, n_header, n_runs, max_rounds, n_bad);
  return n_bad ? 1 : 0;
}
