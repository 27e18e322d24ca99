// zh_inflate_index.h — the member index of a BGZF / multi-member gzip file: where every member starts, how long it is and where its
// output goes, found on the device without decoding anything, so that a whole file becomes the item array of zh_inflate_check.h's three launches.
//
// A HINTED member starts at p (S = the size of the source) when: S - p >= 12; src[p..p+3) = 1f 8b 08; FLG bit 2 (FEXTRA); XLEN = le16(src[p+10]) with
// p + 12 + XLEN <= S; the subfields inside those XLEN bytes (SI1 SI2 SLEN(le16) data), walked from the first, reach one with SI1 'B', SI2 'C', SLEN 2 — a
// subfield whose four header bytes or whose SLEN run past XLEN ends the walk without a hint —; and L = le16(its data) + 1 has L >= 12 + XLEN + 8 and
// p + L <= S. The member is src[p .. p + L), its ISIZE le32(src[p + L - 4]), the next position p + L. Nothing else is looked at: the rest of the header,
// the deflate stream, the CRC and ISIZE itself stay with zh_frame_heads, the inflate kernel and zh_check_members.
// The INDEX is the chain of hinted members from p = 0; it stops at the first p that starts none, with a kind: 0 p == S; 1 magic and CM there but no
// hint (a gzip member the index cannot size); 2 a hint whose L is too short or reaches past S; 3 anything else. Item i = {p_i, L_i, the sum of the
// ISIZEs before it, ISIZE_i}, sums in 64 bits.
//
// The chain is serial: S / (mean member) dependent loads. Here it is speculated per tile of T bytes, verified, and the rare miss walked again:
//
//   zh_ix_tiles    one wave per tile k: the 64 lanes scan [k T, (k + 1) T) for the first position that starts a hinted member — 16-byte loads where
//                  the window lies inside the source, bytes at its two edges —, the tile's GUESS (tile 0: position 0, whatever lies there). A guess
//                  behind the tile's end could never be the chain's entry into this tile, so the candidates end with the tile; the loads of a probe
//                  (a header that straddles the end) run past it, never past S. One lane then hops from the guess until p >= (k + 1) T or a stop and
//                  stores one fixed-size record: guess, exit, stop kind, members, sum of ISIZE. No per-member list: nothing to overflow.
//   zh_ix_resolve  one wave, one lane working: e = 0; tile e / T is confirmed if its guess is e, else it is walked again from e (tiles_rewalked) and its
//                  record overwritten; it gets its entry and its bases (members and output bytes in front of it) and e becomes its exit. Tiles the
//                  chain jumps over stay unused. The pass ends at a stop and writes the totals.
//   zh_ix_items    one lane per used tile: the walk from the tile's entry once more, items[base + i] written.
//
// The walk, the scan and the three passes are templates over a RECORD FORMAT and a range [D0, D1) of the source (here: the whole source); zh_unzip.h walks a ZIP
// archive's central directory with them.
// Dependent loads in a row: about T / (mean member) in the first and the last pass, S / T in the middle one.
// Every result equals the serial walk bit for bit for ANY bytes in src, and no load touches a byte outside src[0 .. S): zh_ix_probe orders its
// loads behind the comparisons that bound them.
#pragma once
#include <stdint.h>

#include "zh_inflate_out.h"

#define ZH_IX_TILE (256u * 1024u)   // bytes per tile (ZULTRA_HIP_INDEX_TILE overrides it per call: any value >= 32)
#define ZH_IX_TILE_MIN 32u
#define ZH_IX_THREADS 64
#define ZH_IX_MEMBER 0xFFu          // zh_ix_probe: a hinted member starts here (no stop)
#define ZH_IX_NOWHERE (~0ull)       // a tile without a guess

typedef struct zh_ix_tile_s {
   uint64_t guess, entry, exit;   // entry: zh_ix_resolve
   uint64_t out_sum, out_base;    // the ISIZEs of the tile's members; of the members in front of the tile (zh_ix_resolve)
   uint64_t member_base;          // (zh_ix_resolve)
   uint32_t members, stop;        // stop: 0..3, or ZH_IX_MEMBER where the walk left the tile
   uint32_t used, pad;            // used: the chain entered this tile (zh_ix_resolve)
} zh_ix_tile_t;

typedef struct zh_ix_totals_s {
   uint64_t members, out_size, src_used;
   uint32_t stop, pad;
   uint64_t tiles, tiles_rewalked;
} zh_ix_totals_t;

#if defined(__HIPCC__) || defined(ZH_EMU)

__device__ __forceinline__ uint32_t zh_ix_le16(const uint8_t *q) { return (uint32_t)q[0] | ((uint32_t)q[1] << 8); }

// What starts at p <= S: ZH_IX_MEMBER with its length and ISIZE, or the stop kind.
__device__ __forceinline__ uint32_t zh_ix_probe(const uint8_t *src, uint64_t S, uint64_t p, uint32_t *len, uint32_t *isize) {
   if (p == S) return 0u;
   const uint8_t *q = src + p;
   if (S - p < 12u || q[0] != 0x1f || q[1] != 0x8b || q[2] != 8) return 3u;
   if (!(q[3] & 4u)) return 1u;
   const uint32_t xlen = zh_ix_le16(q + 10);
   if ((uint64_t)xlen > S - p - 12u) return 1u;
   for (uint32_t at = 0; xlen - at >= 4u;) {   // (at <= xlen throughout)
      const uint8_t *f = q + 12u + at;
      const uint32_t slen = zh_ix_le16(f + 2);
      if (slen > xlen - at - 4u) break;
      if (f[0] == 'B' && f[1] == 'C' && slen == 2u) {
         const uint32_t L = zh_ix_le16(f + 4) + 1u;
         if (L < 12u + xlen + 8u || (uint64_t)L > S - p) return 2u;
         const uint8_t *t = q + L - 4u;
         *len = L;
         *isize = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
         return ZH_IX_MEMBER;
      }
      at += 4u + slen;
   }
   return 1u;
}

// The gzip index as a record format of the tiled chain walk below. A FORMAT F names: item_t, what the last pass writes per record; SIG / SIG_MASK, the
// little-endian bytes a record starts with, and BEHIND, how many bytes of them may lie behind a lane's 16-byte window (their count less one); probe(src, D1,
// p, &len, &val) — what starts at p <= D1, the end of the chain's range: ZH_IX_MEMBER with the record's length and the value the index sums, or a stop kind,
// every load inside [p, D1) —; and put(item, src, p, len, sum, val), item i of a walk, `sum` the values in front of it. zh_unzip.h has the second format.
struct zh_ix_gzip_t {
   typedef zh_inflate_item_t item_t;
   static constexpr uint32_t SIG = 0x088b1fu, SIG_MASK = 0xFFFFFFu, BEHIND = 2u;
   static __device__ __forceinline__ uint32_t probe(const uint8_t *src, uint64_t D1, uint64_t p, uint32_t *len, uint32_t *val) { return zh_ix_probe(src, D1, p, len, val); }
   static __device__ __forceinline__ void put(zh_inflate_item_t *item, const uint8_t *src, uint64_t p, uint32_t len, uint64_t sum, uint32_t val) {
      zh_inflate_item_t it;
      it.src_off = p;
      it.src_size = len;
      it.dst_off = sum;
      it.dst_cap = val;
      *item = it;
   }
};

// The chain from p while p < end (one lane), in src[.. D1). ITEMS: item base + i is written for record i of the walk, with out_base + the values before it.
struct zh_ix_walk_t {
   uint64_t exit, out_sum;
   uint32_t members, stop;
};
template <class F, bool ITEMS>
__device__ __forceinline__ zh_ix_walk_t zh_ix_walk(const uint8_t *src, uint64_t D1, uint64_t p, uint64_t end, typename F::item_t *items, uint64_t out_base) {
   zh_ix_walk_t w;
   w.out_sum = 0;
   w.members = 0;
   w.stop = ZH_IX_MEMBER;
   while (p < end) {
      uint32_t len = 0, val = 0;
      const uint32_t kind = F::probe(src, D1, p, &len, &val);
      if (kind != ZH_IX_MEMBER) {
         w.stop = kind;
         break;
      }
      if (ITEMS) F::put(items + w.members, src, p, len, out_base + w.out_sum, val);
      w.members++;   // (a tile holds fewer than 2^32 records: T < 2^32 * 20 bytes, as the host has seen to)
      w.out_sum += val;
      p += len;
   }
   w.exit = p;
   return w;
}

// Tile k of the chain's range [D0, D1) is [D0 + k T, D0 + (k + 1) T).
__device__ __forceinline__ uint64_t zh_ix_tile_end(uint64_t k, uint64_t T, uint64_t D0, uint64_t D1) {
   const uint64_t from = D0 + k * T;
   return (D1 - from > T) ? from + T : D1 + 1u;   // (the last tile's walk goes on to p == D1, which is a stop)
}

// The first position in [from, to) that starts a record, or ZH_IX_NOWHERE: the whole wave, wave-uniform result. to <= D1 <= S, the size of the source: no
// load touches a byte outside src[0 .. S).
template <class F>
__device__ __forceinline__ uint64_t zh_ix_scan(const uint8_t *src, uint64_t S, uint64_t D1, uint64_t from, uint64_t to) {
   const uint32_t lane = zh_lane();
   const int64_t lead = (int64_t)((uintptr_t)(src + from) & 15u);
   // in round `cb` lane l looks at the sixteen positions [cb + 16 l, cb + 16 l + 16): the window is 16-byte aligned in memory
   for (int64_t cb = (int64_t)from - lead; cb < (int64_t)to; cb += 16 * 64) {
      const int64_t w = cb + 16 * (int64_t)lane;
      uint32_t d[5] = {0u, 0u, 0u, 0u, 0u};
      if (w >= 0 && (uint64_t)w + 16u <= S) {
         const uint4 v = *(const uint4 *)(src + w);
         d[0] = v.x;
         d[1] = v.y;
         d[2] = v.z;
         d[3] = v.w;
      }
      else if (w < (int64_t)S && w + 16 > 0) {   // an edge of the source: its bytes one by one, zeros outside
#pragma unroll
         for (int j = 0; j < 16; j++) {
            const int64_t at = w + j;
            if (at >= 0 && (uint64_t)at < S) d[j >> 2] |= (uint32_t)src[at] << (8 * (j & 3));
         }
      }
      // the BEHIND bytes behind the window: the next lane's first ones; lane 63 loads its own
      d[4] = zh_shfl(d[0], (int)((lane + 1u) & 63u));
      if (lane == 63u) {
         d[4] = 0;
#pragma unroll
         for (int j = 0; j < (int)F::BEHIND; j++) {
            const int64_t at = w + 16 + j;
            if (at >= 0 && (uint64_t)at < S) d[4] |= (uint32_t)src[at] << (8 * j);
         }
      }
      uint32_t mask = 0;
#pragma unroll
      for (int i = 0; i < 16; i++) {
         const uint32_t sig = (i & 3) ? zh_funnel(d[(i >> 2) + 1], d[i >> 2], 8u * (i & 3)) : d[i >> 2];
         if ((sig & F::SIG_MASK) == F::SIG) mask |= 1u << i;
      }
      uint64_t hit = ZH_IX_NOWHERE;
      while (mask) {   // (rare: the lane's candidates in order, each probed in full)
         const int64_t at = w + (__ffs((int)mask) - 1);
         mask &= mask - 1u;
         uint32_t len, val;
         if (at >= (int64_t)from && at < (int64_t)to && F::probe(src, D1, (uint64_t)at, &len, &val) == ZH_IX_MEMBER) {
            hit = (uint64_t)at;
            break;
         }
      }
      const uint64_t any = zh_ballot(hit != ZH_IX_NOWHERE);
      if (any) {   // the lowest lane's is the first of the round
         const int l = zh_ctz64(any);
         const uint32_t lo = zh_shfl((uint32_t)hit, l), hi = zh_shfl((uint32_t)(hit >> 32), l);
         return ((uint64_t)hi << 32) | lo;
      }
   }
   return ZH_IX_NOWHERE;
}

// The three passes over the chain's range [D0, D1) of src[0 .. S), for any format; the kernels below and zh_unzip.h's are these with a format named.
// One wave per tile, striding.
template <class F>
__device__ __forceinline__ void zh_ix_tiles_pass(const uint8_t *src, uint64_t S, uint64_t D0, uint64_t D1, uint64_t T, uint64_t ntiles, zh_ix_tile_t *__restrict__ tiles) {
   for (uint64_t k = blockIdx.x; k < ntiles; k += gridDim.x) {
      const uint64_t from = D0 + k * T, to = (D1 - from > T) ? from + T : D1;
      const uint64_t guess = k == 0 ? D0 : zh_ix_scan<F>(src, S, D1, from, to);
      if (zh_lane() == 0) {
         zh_ix_tile_t r;
         r.guess = guess;
         r.entry = r.out_base = r.member_base = 0;
         r.used = r.pad = 0;
         zh_ix_walk_t w;
         w.exit = ZH_IX_NOWHERE;
         w.out_sum = 0;
         w.members = 0;
         w.stop = ZH_IX_MEMBER;
         if (guess != ZH_IX_NOWHERE) w = zh_ix_walk<F, false>(src, D1, guess, zh_ix_tile_end(k, T, D0, D1), NULL, 0);
         r.exit = w.exit;
         r.out_sum = w.out_sum;
         r.members = w.members;
         r.stop = w.stop;
         tiles[k] = r;
      }
   }
}

// One wave, lane 0 working: the chain of tiles from position D0.
template <class F>
__device__ __forceinline__ void zh_ix_resolve_pass(const uint8_t *src, uint64_t D0, uint64_t D1, uint64_t T, uint64_t ntiles, zh_ix_tile_t *tiles, zh_ix_totals_t *totals) {
   if (blockIdx.x != 0 || threadIdx.x != 0) return;
   zh_ix_totals_t t;
   t.members = t.out_size = t.tiles = t.tiles_rewalked = 0;
   t.stop = 0;
   t.pad = 0;
   uint64_t e = D0;
   for (;;) {
      if (e >= D1) break;   // (e == D1: the range is a complete chain; a walk never passes D1)
      const uint64_t k = (e - D0) / T;   // (< ntiles, as e < D1)
      zh_ix_tile_t r = tiles[k];
      if (r.guess != e) {
         const zh_ix_walk_t w = zh_ix_walk<F, false>(src, D1, e, zh_ix_tile_end(k, T, D0, D1), NULL, 0);
         r.exit = w.exit;
         r.out_sum = w.out_sum;
         r.members = w.members;
         r.stop = w.stop;
         t.tiles_rewalked++;
      }
      r.entry = e;
      r.member_base = t.members;
      r.out_base = t.out_size;
      r.used = 1;
      tiles[k] = r;
      t.members += r.members;
      t.out_size += r.out_sum;
      t.tiles++;
      e = r.exit;   // (> entry unless the walk stopped at once: every record is at least 20 bytes long)
      if (r.stop != ZH_IX_MEMBER) {
         t.stop = r.stop;
         break;
      }
   }
   t.src_used = e;
   *totals = t;
}

// One lane per tile the chain entered: its items, items[member_base ..).
template <class F>
__device__ __forceinline__ void zh_ix_items_pass(const uint8_t *src, uint64_t D0, uint64_t D1, uint64_t T, uint64_t ntiles, const zh_ix_tile_t *__restrict__ tiles, typename F::item_t *__restrict__ items) {
   for (uint64_t k = (uint64_t)blockIdx.x * ZH_IX_THREADS + threadIdx.x; k < ntiles; k += (uint64_t)gridDim.x * ZH_IX_THREADS) {
      const zh_ix_tile_t r = tiles[k];
      if (r.used && r.members) (void)zh_ix_walk<F, true>(src, D1, r.entry, zh_ix_tile_end(k, T, D0, D1), items + r.member_base, r.out_base);
   }
}

// The gzip index: the chain's range is the whole source.
__global__ void __launch_bounds__(ZH_IX_THREADS)
zh_ix_tiles(const uint8_t *src, uint64_t S, uint64_t T, uint64_t ntiles, zh_ix_tile_t *__restrict__ tiles) {
   zh_ix_tiles_pass<zh_ix_gzip_t>(src, S, 0, S, T, ntiles, tiles);
}
__global__ void __launch_bounds__(ZH_IX_THREADS)
zh_ix_resolve(const uint8_t *src, uint64_t S, uint64_t T, uint64_t ntiles, zh_ix_tile_t *tiles, zh_ix_totals_t *totals) {
   zh_ix_resolve_pass<zh_ix_gzip_t>(src, 0, S, T, ntiles, tiles, totals);
}
__global__ void __launch_bounds__(ZH_IX_THREADS)
zh_ix_items(const uint8_t *src, uint64_t S, uint64_t T, uint64_t ntiles, const zh_ix_tile_t *__restrict__ tiles, zh_inflate_item_t *__restrict__ items) {
   zh_ix_items_pass<zh_ix_gzip_t>(src, 0, S, T, ntiles, tiles, items);
}
#endif
