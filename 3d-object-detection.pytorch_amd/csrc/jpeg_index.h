// The host half of the device JPEG decode (include/t3d.h, next to t3d_jpeg_index): parse the markers of a baseline file, walk
// its one entropy-coded scan and record where every seg_mcus-th MCU starts.  No HIP include and no allocation: a stand-alone
// host program compiles this header on its own (tools/jpeg_index_check.cpp runs it under the sanitizers).
// The two halves are two functions: the markers (t3d_jpeg_markers_impl; t3d_jpeg_header is it plus the table check, for files whose
// scan the device walks: csrc/jpeg_scan.h) and the scan walk, which t3d_jpeg_index_impl runs behind the markers.
// What the device decoder shares with it -- the Huffman table expansion and the zig-zag order -- is marked T3D_JPEG_HD.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/t3d.h"

#ifdef __HIPCC__
#define T3D_JPEG_HD __host__ __device__
#else
#define T3D_JPEG_HD
#endif

// zig-zag position -> natural (row-major) position
#define T3D_JPEG_ZIGZAG                                                                                                      \
  {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// One Huffman table, expanded: codes of up to T3D_JPEG_LOOK bits resolve in one lookup (length << 8 | symbol, 0: longer or
// none), longer ones through the canonical maxcode / offset pair of their length.
#define T3D_JPEG_LOOK 9
struct t3d_jpeg_huff {
  uint16_t look[1 << T3D_JPEG_LOOK];
  int32_t maxcode[17];    // [l]: the largest code of length l, -1 when there is none
  int32_t valoff[17];     // [l]: symbol index of a code c of length l = valoff[l] + c
  uint8_t vals[256];
};

// bits[16] + vals (at most `cap` of them) -> *h.  false: more symbols than `cap`, or the lengths do not form a prefix code
// (the all-ones code of a length counts as taken, as in libjpeg).
T3D_JPEG_HD inline bool t3d_jpeg_build_huff(const uint8_t* bits, const uint8_t* vals, int cap, t3d_jpeg_huff* h) {
  for (int i = 0; i < (1 << T3D_JPEG_LOOK); ++i) h->look[i] = 0;
  for (int i = 0; i < 256; ++i) h->vals[i] = 0;
  h->maxcode[0] = -1;
  h->valoff[0] = 0;
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = bits[l - 1];
    h->valoff[l] = k - code;
    for (int j = 0; j < n; ++j, ++k, ++code) {
      if (k >= cap || code >= (1 << l) - 1) return false;
      const uint8_t sym = vals[k];
      h->vals[k] = sym;
      if (l <= T3D_JPEG_LOOK) {
        const int sh = T3D_JPEG_LOOK - l;
        for (int f = 0; f < (1 << sh); ++f) h->look[(code << sh) + f] = (uint16_t)((l << 8) | sym);
      }
    }
    h->maxcode[l] = n ? code - 1 : -1;
    code <<= 1;
  }
  return true;
}

// the symbol of the code at the top of `peek16` (the next 16 bits of the stream) -> length << 8 | symbol, or -1: no such code
T3D_JPEG_HD inline int t3d_jpeg_huff_decode(const t3d_jpeg_huff* h, uint32_t peek16) {
  const int e = h->look[peek16 >> (16 - T3D_JPEG_LOOK)];
  if (e) return e;
  for (int l = T3D_JPEG_LOOK + 1; l <= 16; ++l) {
    const int c = (int)(peek16 >> (16 - l));
    if (c <= h->maxcode[l]) return (l << 8) | h->vals[(h->valoff[l] + c) & 255];
  }
  return -1;
}

// the t extra bits v of a DC difference or AC value -> the value (t = 0: 0)
T3D_JPEG_HD inline int t3d_jpeg_extend(int v, int t) { return t && v < (1 << (t - 1)) ? v - (1 << t) + 1 : v; }

// blocks of one MCU, and of component c in it
T3D_JPEG_HD inline int t3d_jpeg_mcu_blocks(int sampling) { return sampling == T3D_JPEG_GRAY ? 1 : (sampling == T3D_JPEG_444 ? 3 : 6); }

namespace t3d_jpeg_host {

// The scan as a bit stream: a 64-bit window refilled bytewise, FF 00 unstuffed.  At a marker or the end of the data it feeds
// zero bits and counts them, so the caller knows when it has consumed bits that were not there.  The offsets of the last 16
// bytes taken are kept: the position of the first unconsumed bit is the byte taken ceil(cnt / 8) bytes ago.
struct Bits {
  const uint8_t* p;
  long long n, pos;        // the scan and the next byte to take
  uint64_t buf;
  int cnt, fake;           // valid bits in buf (its low end), and how many zero bits were made up in all
  uint32_t ring[16];
  unsigned int taken;

  void init(const uint8_t* scan, long long bytes) {
    p = scan, n = bytes, pos = 0, buf = 0, cnt = 0, fake = 0, taken = 0;
    for (int i = 0; i < 16; ++i) ring[i] = 0;
  }
  void fill() {
    while (cnt <= 56) {
      int b = 0;
      bool real = false;
      if (!fake && pos < n) {
        b = p[pos];
        if (b != 0xFF) {
          real = true;
        } else if (pos + 1 < n && p[pos + 1] == 0) {
          real = true;
        }
      }
      if (real) {
        ring[taken++ & 15] = (uint32_t)pos;
        pos += b == 0xFF ? 2 : 1;
      } else {
        b = 0;
        fake += 8;
        ring[taken++ & 15] = (uint32_t)pos;
      }
      buf = (buf << 8) | (uint64_t)b;
      cnt += 8;
    }
  }
  uint32_t peek16() {
    if (cnt < 16) fill();
    return (uint32_t)(buf >> (cnt - 16)) & 0xFFFFu;
  }
  void skip(int k) { cnt -= k; }
  int get(int k) {       // k <= 16
    if (k == 0) return 0;
    if (cnt < k) fill();
    cnt -= k;
    return (int)((buf >> cnt) & ((1u << k) - 1));
  }
  bool overran() const { return fake > cnt; }           // some made-up bit has been consumed
  // where the first unconsumed bit lies (only meaningful while !overran() and at least one real bit is left or the scan ended)
  void where(uint32_t* byte, int* bit) {
    if (cnt == 0) fill();
    const int back = (cnt + 7) >> 3;
    *byte = ring[(taken - back) & 15];
    *bit = (8 - (cnt & 7)) & 7;
  }
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

}  // namespace t3d_jpeg_host

// The MARKER half of the indexer: everything of *info but scan_bytes (left 0), from the markers up to and including SOS.  Nothing
// of the scan is read.  have_dc / have_ac: which Huffman tables the file defined.
inline int t3d_jpeg_markers_impl(const unsigned char* data, long long bytes, int seg_mcus, t3d_jpeg_info* info, bool have_dc[2],
                                 bool have_ac[2]) {
  using namespace t3d_jpeg_host;
  if (!data || !info || bytes < 0 || seg_mcus < 1) return T3D_ERR_ARG;
  memset(info, 0, sizeof(*info));
  info->seg_mcus = seg_mcus;
  auto unsupported = [&](int reason) {
    info->reason = reason;
    return (int)T3D_ERR_UNSUPPORTED;
  };
  if (bytes < 4 || data[0] != 0xFF || data[1] != 0xD8) return T3D_ERR_ARG;
  static const uint8_t zigzag[64] = T3D_JPEG_ZIGZAG;
  uint8_t qt[4][64];
  bool have_q[4] = {false, false, false, false};
  have_dc[0] = have_dc[1] = have_ac[0] = have_ac[1] = false;
  bool have_sof = false;
  int comp_id[3] = {0, 0, 0}, comp_h[3] = {0, 0, 0}, comp_v[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0};
  int adobe_transform = -1;
  long long pos = 2;
  for (;;) {
    // the next marker: FF, any number of fill FFs, the code
    if (pos + 2 > bytes || data[pos] != 0xFF) return T3D_ERR_ARG;
    while (pos + 1 < bytes && data[pos + 1] == 0xFF) ++pos;
    if (pos + 2 > bytes) return T3D_ERR_ARG;
    const int m = data[pos + 1];
    pos += 2;
    if (m == 0xD9 || m == 0xD8 || m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) return T3D_ERR_ARG;   // no scan yet
    if (pos + 2 > bytes) return T3D_ERR_ARG;
    const int len = be16(data + pos);
    if (len < 2 || pos + len > bytes) return T3D_ERR_ARG;
    const uint8_t* seg = data + pos + 2;
    const int n = len - 2;
    if (m == 0xDB) {                                  // DQT
      int o = 0;
      while (o < n) {
        const int pq = seg[o] >> 4, tq = seg[o] & 15;
        if (tq > 3 || pq > 1) return T3D_ERR_ARG;
        if (pq == 1) return unsupported(T3D_JPEG_REASON_QUANT16);
        if (o + 65 > n) return T3D_ERR_ARG;
        for (int k = 0; k < 64; ++k) qt[tq][zigzag[k]] = seg[o + 1 + k];
        have_q[tq] = true;
        o += 65;
      }
    } else if (m == 0xC4) {                           // DHT
      int o = 0;
      while (o < n) {
        if (o + 17 > n) return T3D_ERR_ARG;
        const int tc = seg[o] >> 4, th = seg[o] & 15;
        if (tc > 1 || th > 1) return T3D_ERR_ARG;     // baseline: two tables of each class
        int cnt = 0;
        for (int k = 0; k < 16; ++k) cnt += seg[o + 1 + k];
        if (cnt > (tc ? 256 : 16) || o + 17 + cnt > n) return T3D_ERR_ARG;
        uint8_t* bits = tc ? info->ac_bits[th] : info->dc_bits[th];
        uint8_t* vals = tc ? info->ac_vals[th] : info->dc_vals[th];
        memcpy(bits, seg + o + 1, 16);
        memset(vals, 0, tc ? 256 : 16);
        memcpy(vals, seg + o + 17, cnt);
        (tc ? have_ac : have_dc)[th] = true;
        o += 17 + cnt;
      }
    } else if (m == 0xC0) {                           // SOF0
      if (have_sof || n < 6) return T3D_ERR_ARG;
      const int prec = seg[0], nc = seg[5];
      info->h = be16(seg + 1), info->w = be16(seg + 3), info->ncomp = nc;
      if (n != 6 + 3 * nc) return T3D_ERR_ARG;
      if (prec != 8) return unsupported(T3D_JPEG_REASON_PRECISION);
      if (info->h < 1 || info->w < 1) return T3D_ERR_ARG;      // (h = 0: the height comes in a DNL marker -- not baseline practice)
      if (nc != 1 && nc != 3) return nc == 0 ? (int)T3D_ERR_ARG : unsupported(T3D_JPEG_REASON_COMPONENTS);
      for (int c = 0; c < nc; ++c) {
        comp_id[c] = seg[6 + 3 * c], comp_h[c] = seg[7 + 3 * c] >> 4, comp_v[c] = seg[7 + 3 * c] & 15, comp_tq[c] = seg[8 + 3 * c];
        if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4 || comp_tq[c] > 3) return T3D_ERR_ARG;
      }
      if (nc == 1) {
        info->sampling = T3D_JPEG_GRAY;               // (a single component is never interleaved: its factors do not matter)
      } else {
        const bool c11 = comp_h[1] == 1 && comp_v[1] == 1 && comp_h[2] == 1 && comp_v[2] == 1;
        if (c11 && comp_h[0] == 1 && comp_v[0] == 1) info->sampling = T3D_JPEG_444;
        else if (c11 && comp_h[0] == 2 && comp_v[0] == 2) info->sampling = T3D_JPEG_420;
        else return unsupported(T3D_JPEG_REASON_SAMPLING);
        if (comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return unsupported(T3D_JPEG_REASON_COLOURSPACE);
      }
      have_sof = true;
    } else if (m >= 0xC1 && m <= 0xCF && m != 0xC8) { // every other frame type (C4 was DHT; CC = DAC: arithmetic conditioning)
      if (n >= 1 && m != 0xCC && seg[0] != 8) return unsupported(T3D_JPEG_REASON_PRECISION);
      return unsupported(T3D_JPEG_REASON_SOF);
    } else if (m == 0xDD) {                           // DRI
      if (n != 2) return T3D_ERR_ARG;
      if (be16(seg) != 0) return unsupported(T3D_JPEG_REASON_RESTART);
    } else if (m == 0xEE) {                           // APP14: Adobe's colour transform flag
      if (n >= 12 && memcmp(seg, "Adobe", 5) == 0) adobe_transform = seg[11];
    } else if (m == 0xDA) {                           // SOS
      if (!have_sof || n < 1) return T3D_ERR_ARG;
      const int ns = seg[0];
      if (ns < 1 || ns > 4 || n != 4 + 2 * ns) return T3D_ERR_ARG;
      if (ns != info->ncomp) return unsupported(T3D_JPEG_REASON_SCANS);
      for (int c = 0; c < ns; ++c) {
        if (seg[1 + 2 * c] != comp_id[c]) return unsupported(T3D_JPEG_REASON_SCANS);     // (components out of frame order)
        const int td = seg[2 + 2 * c] >> 4, ta = seg[2 + 2 * c] & 15;
        if (td > 1 || ta > 1 || !have_dc[td] || !have_ac[ta] || !have_q[comp_tq[c]]) return T3D_ERR_ARG;
        info->comp_dc[c] = (uint8_t)td, info->comp_ac[c] = (uint8_t)ta;
        memcpy(info->quant[c], qt[comp_tq[c]], 64);
      }
      if (seg[1 + 2 * ns] != 0 || seg[2 + 2 * ns] != 63 || seg[3 + 2 * ns] != 0) return T3D_ERR_ARG;    // Ss, Se, Ah/Al of baseline
      if (info->ncomp == 3 && adobe_transform == 0) return unsupported(T3D_JPEG_REASON_COLOURSPACE);
      pos += len;
      break;
    }
    // (APPn, COM and whatever else carries a length: skipped)
    pos += len;
  }

  const int mcu_px = info->sampling == T3D_JPEG_420 ? 16 : 8;
  info->mcus_x = (info->w + mcu_px - 1) / mcu_px, info->mcus_y = (info->h + mcu_px - 1) / mcu_px;
  const long long nmcu = (long long)info->mcus_x * info->mcus_y;
  const long long nseg = (nmcu + seg_mcus - 1) / seg_mcus;
  if (nseg > 0x7FFFFFFF) return T3D_ERR_ARG;
  info->nseg = (int)nseg;
  info->scan_offset = pos;
  if (bytes - pos > 0xFFFFFFFFll) return T3D_ERR_ARG;      // (t3d_jpeg_seg.byte is 32 bits)
  return T3D_OK;
}

// the file's Huffman tables expanded -> false: one of them is no prefix code
inline bool t3d_jpeg_file_tables(const t3d_jpeg_info* info, const bool have_dc[2], const bool have_ac[2], t3d_jpeg_huff dc[2],
                                 t3d_jpeg_huff ac[2]) {
  for (int t = 0; t < 2; ++t) {
    if (have_dc[t] && !t3d_jpeg_build_huff(info->dc_bits[t], info->dc_vals[t], 16, &dc[t])) return false;
    if (have_ac[t] && !t3d_jpeg_build_huff(info->ac_bits[t], info->ac_vals[t], 256, &ac[t])) return false;
  }
  return true;
}

// include/t3d.h: t3d_jpeg_header
inline int t3d_jpeg_header_impl(const unsigned char* data, long long bytes, int seg_mcus, t3d_jpeg_info* info) {
  bool have_dc[2], have_ac[2];
  const int rc = t3d_jpeg_markers_impl(data, bytes, seg_mcus, info, have_dc, have_ac);
  if (rc != T3D_OK) return rc;
  t3d_jpeg_huff dc[2], ac[2];
  if (!t3d_jpeg_file_tables(info, have_dc, have_ac, dc, ac)) return T3D_ERR_ARG;
  info->scan_bytes = bytes - info->scan_offset;            // the clamp: the scan's length is the scan walk's to find
  return T3D_OK;
}

// include/t3d.h: t3d_jpeg_index
inline int t3d_jpeg_index_impl(const unsigned char* data, long long bytes, int seg_mcus, t3d_jpeg_info* info, t3d_jpeg_seg* segs,
                               long long seg_capacity) {
  using namespace t3d_jpeg_host;
  if (segs && seg_capacity < 0) return T3D_ERR_ARG;
  bool have_dc[2], have_ac[2];
  const int rc = t3d_jpeg_markers_impl(data, bytes, seg_mcus, info, have_dc, have_ac);
  if (rc != T3D_OK) return rc;
  auto unsupported = [&](int reason) {
    info->reason = reason;
    return (int)T3D_ERR_UNSUPPORTED;
  };
  // ---- the scan ----
  const long long pos = info->scan_offset;
  const long long nmcu = (long long)info->mcus_x * info->mcus_y;
  if (segs && seg_capacity < info->nseg) return T3D_ERR_ARG;
  t3d_jpeg_huff dc[2], ac[2];
  if (!t3d_jpeg_file_tables(info, have_dc, have_ac, dc, ac)) return T3D_ERR_ARG;
  Bits br;
  br.init(data + pos, bytes - pos);
  int pred[3] = {0, 0, 0};
  const int nblk[3] = {info->sampling == T3D_JPEG_420 ? 4 : 1, 1, 1};
  for (long long mcu = 0; mcu < nmcu; ++mcu) {
    if (mcu % seg_mcus == 0) {
      uint32_t byte;
      int bit;
      br.where(&byte, &bit);
      if (br.overran() || br.fake >= br.cnt) return T3D_ERR_ARG;     // no real bit left for this MCU
      if (segs) {
        t3d_jpeg_seg& s = segs[mcu / seg_mcus];
        s.byte = byte, s.bit = (uint8_t)bit, s.reserved = 0, s.mcu = (int)mcu;
        for (int c = 0; c < 3; ++c) s.pred[c] = (short)pred[c];
      }
    }
    for (int c = 0; c < info->ncomp; ++c) {
      const t3d_jpeg_huff* hd = &dc[info->comp_dc[c]];
      const t3d_jpeg_huff* ha = &ac[info->comp_ac[c]];
      for (int b = 0; b < nblk[c]; ++b) {
        int e = t3d_jpeg_huff_decode(hd, br.peek16());
        if (e < 0) return T3D_ERR_ARG;
        br.skip(e >> 8);
        const int t = e & 255;
        if (t > 11) return T3D_ERR_ARG;                               // a DC category beyond 8-bit baseline
        pred[c] += t3d_jpeg_extend(br.get(t), t);
        if (pred[c] < -32768 || pred[c] > 32767) return T3D_ERR_ARG;  // (the segment table holds int16)
        for (int k = 1; k < 64;) {
          e = t3d_jpeg_huff_decode(ha, br.peek16());
          if (e < 0) return T3D_ERR_ARG;
          br.skip(e >> 8);
          const int r = (e >> 4) & 15, s = e & 15;
          if (s == 0) {
            if (r != 15) break;                                        // EOB
            k += 16;
            if (k > 64) return T3D_ERR_ARG;                            // ZRL past the block (k == 64: the block is full)
            continue;
          }
          k += r;
          if (k > 63) return T3D_ERR_ARG;
          br.get(s);
          ++k;
        }
        if (br.overran()) return T3D_ERR_ARG;                          // a marker or the end of the data inside the scan
      }
    }
  }
  // behind the last MCU: the rest of its byte, then a marker -- EOI
  uint32_t byte;
  int bit;
  br.where(&byte, &bit);
  long long end = byte;                             // (every real bit consumed: where the reader stopped)
  if (bit) end += data[pos + byte] == 0xFF ? 2 : 1; // (a padded FF carries its stuffed 00)
  long long q = pos + end;
  if (q + 2 > bytes || data[q] != 0xFF) return T3D_ERR_ARG;
  while (q + 1 < bytes && data[q + 1] == 0xFF) ++q;
  if (q + 2 > bytes) return T3D_ERR_ARG;
  if (data[q + 1] != 0xD9) {
    const int m = data[q + 1];
    if (m == 0xDA || m == 0xC4 || m == 0xDB) return unsupported(T3D_JPEG_REASON_SCANS);
    return T3D_ERR_ARG;
  }
  info->scan_bytes = end;
  return T3D_OK;
}
