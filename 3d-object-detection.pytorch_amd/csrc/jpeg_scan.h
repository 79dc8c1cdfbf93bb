// What ONE LANE of the device JPEG indexer does (csrc/jpeg_scan.hip launches it; include/t3d.h next to t3d_jpeg_index_device
// states the method): the checked per-image geometry, the state that crosses a subsequence boundary, the bit reader that knows
// where in the STUFFED scan its first unconsumed bit lies, the decode of one subsequence (passes speculate, settle and emit are
// this one function), the steps of a settle round, the trailer check.
// The yardstick is the host indexer of csrc/jpeg_index.h: the rows, scan_bytes and accept / refuse are its, for every file.
// Like csrc/jpeg_decode.h it has no HIP include, so the very code the kernels run also compiles for the host, where
// tools/jpeg_scan_check.cpp runs the lanes in a loop (tests/test_jpeg_scan_host.py; under the address and undefined-behaviour
// sanitizers by hand).
#pragma once
#include "jpeg_decode.h"

namespace t3d_jpeg_scan {

typedef unsigned long long u64;
using t3d_jpeg_lane::lo;

// ---- the state that crosses a boundary ---------------------------------------------------------------------------------------
// The next symbol begins at bit `bit` (0 = the most significant) of byte `byte` of the stuffed scan (never a stuffed 00; the
// position of the marker or of the data's end when every real bit is consumed), in block slot `blk` of its MCU, at zig-zag
// position k (0: a DC code is expected).  bits 0..31 byte, 32..34 bit, 35..37 blk, 38..44 k; kInvalid: no valid state (the
// stream ended upstream); kDirty (entries only): the lane has to decode again in this round.
constexpr u64 kInvalid = 1ull << 62, kDirty = 1ull << 63;
T3D_JPEG_LANE u64 pack(u64 byte, int bit, int blk, int k) { return byte | ((u64)bit << 32) | ((u64)blk << 35) | ((u64)k << 38); }
T3D_JPEG_LANE unsigned int state_byte(u64 s) { return (unsigned int)(s & 0xFFFFFFFFull); }
T3D_JPEG_LANE int state_bit(u64 s) { return (int)(s >> 32) & 7; }
T3D_JPEG_LANE int state_blk(u64 s) { return (int)(s >> 35) & 7; }
T3D_JPEG_LANE int state_k(u64 s) { return (int)(s >> 38) & 127; }

// work: one Head an image, then one Rec a subsequence (32 bytes each)
struct alignas(16) Rec {
  u64 entry, exit;               // the state the lane last decoded from, and the one it handed on
  unsigned int mcus;             // MCU starts the lane owns; after the count pass: those in front of it
  unsigned int dc[3];            // the sum of its DC differences per component (wrapping); after the count pass: the predictors at its entry
};
struct alignas(16) Head {
  int err;                       // emit: a check failed before the end of the last MCU
  int rounds;                    // settle rounds used (the timing tool reads it)
  long long end;                 // emit: the scan's length when the trailer is in order, else -1
  long long pad[2];
};
static_assert(sizeof(Rec) == 32 && sizeof(Head) == 32, "include/t3d.h: 32 bytes a record");

// What the kernels need of one image, or ok == false.  Every field is checked here, by every kernel, before it is used.
struct Img {
  bool ok;
  int ncomp, bpm, ybl, nmcu, seg_mcus, nseg;     // bpm: blocks per MCU, ybl: luma blocks of one
  const unsigned char* scan;
  unsigned int n;                // the clamp: bytes from the scan's first to the file's last
  long long nsub;
  t3d_jpeg_seg* segs;
  Rec* recs;
  Head* head;
};

T3D_JPEG_LANE Img image(const unsigned char* data, long long data_bytes, const t3d_jpeg_info* info, t3d_jpeg_seg* segs, long long total_segs,
                        const t3d_jpeg_item& it, int sub, void* work, long long work_bytes, int B, int img) {
  Img g;
  g.ok = false;
  g.ncomp = info->ncomp, g.seg_mcus = info->seg_mcus, g.nseg = info->nseg;
  g.bpm = g.ybl = g.nmcu = 0, g.scan = nullptr, g.n = 0, g.nsub = 0, g.segs = nullptr, g.recs = nullptr, g.head = nullptr;
  const int h = info->h, w = info->w, sampling = info->sampling;
  if (h < 1 || w < 1 || h > 65535 || w > 65535) return g;
  if (sampling != T3D_JPEG_GRAY && sampling != T3D_JPEG_444 && sampling != T3D_JPEG_420) return g;
  if (g.ncomp != (sampling == T3D_JPEG_GRAY ? 1 : 3)) return g;
  const int px = sampling == T3D_JPEG_420 ? 16 : 8;
  if (info->mcus_x != (w + px - 1) / px || info->mcus_y != (h + px - 1) / px) return g;
  g.nmcu = info->mcus_x * info->mcus_y;                                     // <= 8192 * 8192
  if (g.seg_mcus < 1 || g.nseg != (int)(((long long)g.nmcu + g.seg_mcus - 1) / g.seg_mcus)) return g;
  for (int c = 0; c < g.ncomp; ++c)
    if (info->comp_dc[c] > 1 || info->comp_ac[c] > 1) return g;
  const long long so = info->scan_offset;
  if (it.file_offset < 0 || it.file_bytes < 0 || it.file_offset > data_bytes || it.file_bytes > data_bytes - it.file_offset) return g;
  if (so < 0 || so > it.file_bytes || it.file_bytes - so > 0xFFFFFFFFll) return g;
  if (it.seg_offset < 0 || it.seg_offset > total_segs || g.nseg > total_segs - it.seg_offset) return g;
  const long long n = it.file_bytes - so, nsub = (n + sub - 1) / sub, total_recs = work_bytes / 32 - B;
  if (it.block_offset < 0 || it.block_offset > total_recs || nsub > total_recs - it.block_offset) return g;
  g.bpm = t3d_jpeg_mcu_blocks(sampling), g.ybl = sampling == T3D_JPEG_420 ? 4 : 1;
  g.scan = data + it.file_offset + so;
  g.n = (unsigned int)n, g.nsub = nsub;
  g.segs = segs + it.seg_offset;
  g.head = reinterpret_cast<Head*>(work) + img;
  g.recs = reinterpret_cast<Rec*>(work) + B + it.block_offset;
  g.ok = true;
  return g;
}

// ---- the reader --------------------------------------------------------------------------------------------------------------
// t3d_jpeg_lane::Bits with a position: a 64-bit window (valid bits at its low end), refilled when 24 bits or fewer are left with
// up to four stream bytes that were loaded together; FF 00 is one data byte FF; FF + anything else, or the clamp, stops the
// reader for good: from there it feeds zero bits, counted in `fake` (the host reader's convention).  (cur, bit): where the
// first unconsumed bit lies in the stuffed scan.  A consumed byte is still in the window when the position steps over it
// (cnt + bit <= 63), and it took two raw bytes exactly when it is FF.
struct Reader {
  const unsigned char* p;
  unsigned int n;
  u64 pos, cur, buf;
  int cnt, fake, bit;
  bool stopped;

  T3D_JPEG_LANE unsigned int at(u64 i) const { return i < n ? p[i] : 0xFFu; }      // (behind the clamp: a marker)
  T3D_JPEG_LANE void refill() {
    while (cnt <= 24) {
      if (stopped) {
        buf <<= 32;
        cnt += 32, fake += 32;
        break;
      }
      unsigned int b[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) b[i] = at(pos + i);
      int used = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (used > i || stopped) continue;              // a stuffed 00 that went with its FF
        if (b[i] == 0xFFu) {
          if (b[i + 1] != 0u) {
            stopped = true;
            continue;
          }
          used = i + 2;
        } else {
          used = i + 1;
        }
        buf = (buf << 8) | b[i];
        cnt += 8;
      }
      pos += used;
    }
  }
  T3D_JPEG_LANE void start(const unsigned char* scan, unsigned int bytes, unsigned int byte, int at_bit) {
    p = scan, n = bytes, pos = cur = byte, buf = 0, cnt = 0, fake = 0, bit = at_bit, stopped = false;
    refill();
    cnt -= bit;                                         // (the first refill took at least one byte, or stopped and made 32 bits)
  }
  T3D_JPEG_LANE bool empty() const { return fake >= cnt; }          // no real bit is left
  T3D_JPEG_LANE bool overran() const { return fake > cnt; }         // some made-up bit has been consumed
  T3D_JPEG_LANE unsigned int peek16() const { return (unsigned int)(buf >> (cnt - 16)) & 0xFFFFu; }    // cnt >= 16
  T3D_JPEG_LANE void skip(int k) {                      // k <= 16 <= cnt
    cnt -= k, bit += k;
    while (bit >= 8) {
      cur += ((buf >> (cnt + bit - 8)) & 0xFFu) == 0xFFu ? 2 : 1;
      bit -= 8;
    }
  }
  T3D_JPEG_LANE int get(int k) {                        // k <= 16 <= cnt
    const int v = (int)((unsigned int)(buf >> (cnt - k)) & ((1u << k) - 1u));
    skip(k);
    return v;
  }
};

// lane j's entry for the speculate pass: an MCU begins at its first byte (behind a stuffed 00); lane 0's is true
T3D_JPEG_LANE u64 guess(const Img& g, long long j, int sub) {
  u64 b = (u64)j * (u64)sub;
  if (b > 0 && b < g.n && g.scan[b] == 0 && g.scan[b - 1] == 0xFF) ++b;
  return pack(b, 0, 0, 0);
}

// Behind the last MCU, which ends in front of bit `bit` of byte `byte`: the rest of that byte, then a marker -- EOI, fill FFs
// allowed (the host indexer's lines).  -> the scan's length, or -1.  Every read is inside the clamp.
T3D_JPEG_LANE long long trailer(const Img& g, u64 byte, int bit) {
  long long end = (long long)byte;
  if (bit) end += (byte < g.n ? g.scan[byte] : 0xFF) == 0xFF ? 2 : 1;      // (a padded FF carries its stuffed 00)
  long long q = end;
  const long long n = g.n;
  if (q + 2 > n || g.scan[q] != 0xFF) return -1;
  while (q + 1 < n && g.scan[q + 1] == 0xFF) ++q;
  if (q + 2 > n) return -1;
  return g.scan[q + 1] == 0xD9 ? end : -1;
}

struct Tally { unsigned int mcus, dc[3]; };            // what a lane counts: the MCU starts it owns, its DC differences
struct Truth { unsigned int m; int pred[3]; };         // what emit knows at a lane's entry: MCU starts in front of it, the predictors

// Lane j of a checked image from entry state `in`: every symbol whose first bit lies in the raw bytes [j * sub, (j + 1) * sub) of
// the scan, up to the clamp.  tab: DC 0, DC 1, AC 0, AC 1.  -> the exit state: where the first symbol of a later lane begins, `in`
// itself when that symbol begins behind the lane; kInvalid where a symbol took bits behind a marker or the data's end.
// *t: the lane's counts.
// The exit is a FUNCTION of the entry whatever the bytes are, which is all the settle rounds need.  So that wrong entries fall into
// step with the true decode instead of handing "no valid state" down the chain, a speculative decode RECOVERS from what the host
// indexer refuses: a code that does not exist costs one bit, a DC category above 11 carries no extra bits, a run past coefficient 63
// ends its block; and an entry that is kInvalid, or lies in front of the lane (an earlier lane stopped at a marker), is replaced
// by the lane's own guess.  In a file the host accepts none of this happens on the true chain before the last MCU ends.
// EMIT (tr: the truth at the entry) is the same walk that trusts nothing of it: it ends at the first thing the host indexer
// refuses and sets the image's err (all of it lies before the end of the last MCU, because the lane stops where MCU nmcu would
// begin: there it makes the trailer check and records the scan's length); on the way it writes the row of every MCU m that begins
// here with m % seg_mcus == 0.
// A step consumes at least one bit, or the lane ends: at most 8 * (sub + 4) + 32 steps.
template <bool EMIT>
T3D_JPEG_LANE u64 run(const Img& g, const t3d_jpeg_huff* tab, const int dci[3], const int aci[3], long long j, int sub, u64 in, Tally* t,
                      Truth* tr) {
  t->mcus = t->dc[0] = t->dc[1] = t->dc[2] = 0;
  const u64 hi = lo((u64)(j + 1) * (u64)sub, (u64)g.n);
  if ((in & kInvalid) || state_byte(in) < (u64)j * (u64)sub) {
    if (EMIT) return kInvalid;                          // the true chain ended in front of this lane
    in = guess(g, j, sub);
  }
  if (state_byte(in) >= hi) return in;                  // the lane owns no symbol
  int blk = state_blk(in), k = state_k(in);
  if (blk >= g.bpm || k > 63) return kInvalid;          // (no decode writes such a state)
  unsigned int m = EMIT ? tr->m : 0u;
  if (EMIT && m > (unsigned int)g.nmcu) return in;      // behind the last MCU: not trusted
  Reader r;
  r.start(g.scan, g.n, state_byte(in), state_bit(in));
  for (;;) {
    if (r.cur >= hi) break;                             // the next symbol is a later lane's
    r.refill();
    if (blk == 0 && k == 0) {                           // an MCU begins
      if (EMIT) {
        if (m == (unsigned int)g.nmcu) {
          g.head->end = trailer(g, r.cur, r.bit);
          return kInvalid;
        }
        const unsigned int row = m / (unsigned int)g.seg_mcus;
        if (!r.empty() && m % (unsigned int)g.seg_mcus == 0 && row < (unsigned int)g.nseg) {
          t3d_jpeg_seg s;
          s.byte = (unsigned int)r.cur, s.bit = (unsigned char)r.bit, s.reserved = 0, s.mcu = (int)m;
          for (int c = 0; c < 3; ++c) s.pred[c] = (short)tr->pred[c];
          g.segs[row] = s;
        }
      }
      if (!r.empty()) ++m, ++t->mcus;
    }
    if (r.empty()) {                                    // a marker or the end of the data: in front of MCU nmcu, inside the scan
      if (EMIT) g.head->err = 1;
      break;
    }
    const int c = blk < g.ybl ? 0 : blk - g.ybl + 1;
    bool bad = false;                                   // the host indexer refuses the file here
    if (k == 0) {
      const int e = t3d_jpeg_huff_decode(tab + dci[c], r.peek16());
      if (e < 0) {                                      // no such code
        bad = true;
        r.skip(1);
      } else {
        r.skip(e >> 8);
        const int cat = e & 255;
        if (cat > 11) {                                 // a DC category beyond 8-bit baseline
          bad = true;
        } else {
          r.refill();
          const int d = t3d_jpeg_extend(r.get(cat), cat);
          t->dc[c] += (unsigned int)d;
          if (EMIT) {
            tr->pred[c] += d;                           // (exact: the predictors were inside int16 up to here, |d| <= 2047)
            bad = tr->pred[c] < -32768 || tr->pred[c] > 32767;
          }
        }
        k = 1;
      }
    } else {
      const int e = t3d_jpeg_huff_decode(tab + aci[c], r.peek16());
      if (e < 0) {
        bad = true;
        r.skip(1);
      } else {
        r.skip(e >> 8);
        const int rr = (e >> 4) & 15, sz = e & 15;
        if (sz == 0) {
          k = rr != 15 ? 64 : k + 16;                   // EOB; ZRL (k == 64: the block is full)
          bad = k > 64;
        } else {
          k += rr;
          bad = k > 63;
          if (!bad) {
            r.refill();
            r.skip(sz);
            ++k;
          }
        }
      }
    }
    if (r.overran()) {                                  // the symbol took bits behind a marker or the data's end
      if (EMIT) g.head->err = 1;
      return kInvalid;
    }
    if (bad && EMIT) {
      g.head->err = 1;
      return kInvalid;
    }
    if (k >= 64) {
      k = 0;
      if (++blk == g.bpm) blk = 0;
    }
  }
  return pack(r.cur, r.bit, blk, k);
}

// ---- one settle round, lane by lane -------------------------------------------------------------------------------------------
// take (all lanes, then a barrier): lane j >= 1 looks at its predecessor's exit; -> true when it differs from the entry the lane
// last decoded from, which is then replaced and marked.  again (all lanes, then a barrier): a marked lane decodes from its new entry.
// When no lane took anything, every entry is its predecessor's exit and lane 0's is true: the chain is the sequential decode.
T3D_JPEG_LANE bool take(Rec* recs, long long j) {
  const u64 e = recs[j - 1].exit;
  if (e == (recs[j].entry & ~kDirty)) return false;
  recs[j].entry = e | kDirty;
  return true;
}

T3D_JPEG_LANE void decode_into(const Img& g, const t3d_jpeg_huff* tab, const int dci[3], const int aci[3], long long j, int sub, u64 entry) {
  Tally t;
  Rec& rec = g.recs[j];
  rec.entry = entry;
  rec.exit = run<false>(g, tab, dci, aci, j, sub, entry, &t, nullptr);
  rec.mcus = t.mcus, rec.dc[0] = t.dc[0], rec.dc[1] = t.dc[1], rec.dc[2] = t.dc[2];
}

T3D_JPEG_LANE void again(const Img& g, const t3d_jpeg_huff* tab, const int dci[3], const int aci[3], long long j, int sub) {
  const u64 e = g.recs[j].entry;
  if (e & kDirty) decode_into(g, tab, dci, aci, j, sub, e & ~kDirty);
}

// emit, lane j: the record holds the true entry and, after the count pass, the truth in front of the lane
T3D_JPEG_LANE void emit(const Img& g, const t3d_jpeg_huff* tab, const int dci[3], const int aci[3], long long j, int sub) {
  const Rec rec = g.recs[j];
  Tally t;
  Truth tr;
  tr.m = rec.mcus, tr.pred[0] = (int)rec.dc[0], tr.pred[1] = (int)rec.dc[1], tr.pred[2] = (int)rec.dc[2];
  run<true>(g, tab, dci, aci, j, sub, rec.entry, &t, &tr);
}

}  // namespace t3d_jpeg_scan
