// zh_inflate_range.h — a byte range of a BGZF / multi-member gzip file: which members of the index of zh_inflate_index.h cover bytes [lo, hi) of
// the concatenated output, their items with the destination rebased to the range, and the two slices of the members that straddle an end of it.
//
// The tile records of a resolved index carry member_base and out_base, prefix sums over the members and the output bytes in front of a tile. out_base ascends
// over the tiles the chain entered (`used`); a tile of empty members shares its out_base with the next one. So the member that holds byte x < F, F the sum of
// all ISIZEs, lies in the LAST used tile with out_base <= x: a tile behind the holder starts above x, and an empty tile at or below x has the holder behind it.
//
//   zh_rg_select   one wave: the lanes load 64 tile records a round, coalesced, ballots find the last used tile with out_base <= lo and the same for hi - 1, and the
//                  scan ends behind the first used tile above hi - 1. Lane 0 then walks the first of the two tiles from its true entry, member by member, to
//                  the first member with bytes of its own that reaches past lo; lane 1 does the same for hi - 1. Each writes its half of the plan record.
//   zh_rg_items    one lane per tile from the first to the last selected: the items pass of the index over members m0 .. m1 only, item (member - m0). A
//                  member that lies WHOLLY inside [lo, hi) gets dst_off less lo: it decodes straight into its place in the range. The members that straddle
//                  lo or hi — two at the most, one where the range lies inside a member — get a destination in a buffer of the call's own, the edge buffer,
//                  where they are decoded in full and checked like every other. One batch, one inflate launch: the destination the three launches are
//                  given is the lower of the two buffers' addresses, and an item's dst_off counts from there.
//   zh_rg_edges    behind the check kernel: moves the slice [from, to) of each straddling member out of the edge buffer into the range with zh_copy.h's
//                  mover: a wave per slice of ZH_ZIP_SLICE_CHUNKS chunks, edges bytewise. Only what the member has decoded is moved.
//
// Every load of the tile records and of src is one the index makes too; the edge buffer is 16-byte aligned at both ends, so the mover's aligned loads stay in it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "zh_copy.h"
#include "zh_inflate_check.h"
#include "zh_inflate_index.h"

#define ZH_RG_THREADS 64
#define ZH_RG_ROUND 4u             // 16-byte loads a lane makes in a round of zh_rg_select: 64 tile records
#define ZH_RG_MAX_YSLICES 256u

typedef struct zh_rg_end_s {       // the member that holds one end of the range
   uint64_t member, out_off;       // its number in the index; the output bytes in front of it
   uint64_t src_off, tile;
   uint32_t src_size, isize;
   uint32_t found, pad;            // 0: no such member (an index that does not hold the byte: never)
} zh_rg_end_t;
typedef struct zh_rg_plan_s {
   zh_rg_end_t end[2];             // of lo, of hi - 1
} zh_rg_plan_t;

typedef struct zh_rg_edge_s {      // output bytes [from, to) of the member decoded at buf_at of the edge buffer go to dst + dst_at; to == from: no such edge
   uint64_t buf_at, from, to, dst_at;
   uint64_t slot;                  // its item in the batch
} zh_rg_edge_t;

#if defined(__HIPCC__) || defined(ZH_EMU)

// the highest lane of a ballot (m != 0)
__device__ __forceinline__ uint32_t zh_rg_top(uint64_t m) {
   const uint32_t hi = (uint32_t)(m >> 32);
   return hi ? 63u - (uint32_t)zh_clz32(hi) : 31u - (uint32_t)zh_clz32((uint32_t)m);
}

// One lane: the member of tile t that holds output byte x, from the tile's true entry.
__device__ __forceinline__ zh_rg_end_t zh_rg_find(const uint8_t *src, uint64_t S, const zh_ix_tile_t *tiles, uint64_t t, uint64_t x) {
   zh_rg_end_t e;
   e.member = e.out_off = e.src_off = 0;
   e.tile = t;
   e.src_size = e.isize = e.found = e.pad = 0;
   if (t == ZH_IX_NOWHERE) return e;
   const zh_ix_tile_t r = tiles[t];
   uint64_t p = r.entry, sum = r.out_base;
   for (uint32_t i = 0; i < r.members; i++) {
      const zh_ix_walk_t w = zh_ix_walk<zh_ix_gzip_t, false>(src, S, p, p + 1u, NULL, 0);   // one hop
      if (w.stop != ZH_IX_MEMBER) break;
      if (w.out_sum && sum + w.out_sum > x) {
         e.member = r.member_base + i;
         e.out_off = sum;
         e.src_off = p;
         e.src_size = (uint32_t)(w.exit - p);
         e.isize = (uint32_t)w.out_sum;
         e.found = 1;
         break;
      }
      sum += w.out_sum;
      p = w.exit;
   }
   return e;
}

// One wave. lo <= last < F, the output bytes of the index. A round is 64 tile records, 4 KiB, in four coalesced loads of 16 bytes a lane: in load j lane l holds
// quarter l & 3 of record base + 16 j + (l >> 2) — quarter 2 is {out_base, member_base}, quarter 3 {members, stop, used, pad} —, so the lane of quarter 2 takes
// `used` from its neighbour and votes for its record.
static_assert(sizeof(zh_ix_tile_t) == 64 && offsetof(zh_ix_tile_t, out_base) == 32 && offsetof(zh_ix_tile_t, used) == 56, "the quarters of a tile record");
__global__ void __launch_bounds__(ZH_RG_THREADS)
zh_rg_select(const uint8_t *src, uint64_t S, uint64_t ntiles, const zh_ix_tile_t *__restrict__ tiles, uint64_t lo, uint64_t last, zh_rg_plan_t *plan) {
   if (blockIdx.x != 0) return;
   const uint32_t lane = zh_lane();
   const uint4 *quarters = (const uint4 *)tiles;   // (16-byte aligned: the records are an allocation of their own)
   uint64_t t_lo = ZH_IX_NOWHERE, t_last = ZH_IX_NOWHERE;
   for (uint64_t base = 0; base < ntiles; base += 64u) {
      uint4 v[ZH_RG_ROUND];
#pragma unroll
      for (uint32_t j = 0; j < ZH_RG_ROUND; j++) {   // all of a round's loads in flight before its first ballot
         const uint64_t q = 4u * base + 64u * j + lane;
         v[j] = q < 4u * ntiles ? quarters[q] : make_uint4(0, 0, 0, 0);
      }
      bool past = false;
#pragma unroll
      for (uint32_t j = 0; j < ZH_RG_ROUND; j++) {
         const uint32_t used = zh_shfl(v[j].z, (int)((lane + 1u) & 63u));
         const uint64_t out_base = ((uint64_t)v[j].y << 32) | v[j].x;
         const bool mine = (lane & 3u) == 2u && used != 0;   // (a record behind the last one is zeros: unused)
         const uint64_t b_lo = zh_ballot(mine && out_base <= lo), b_last = zh_ballot(mine && out_base <= last);
         if (b_lo) t_lo = base + 16u * j + (zh_rg_top(b_lo) >> 2);
         if (b_last) t_last = base + 16u * j + (zh_rg_top(b_last) >> 2);
         past = past || zh_ballot(mine && out_base > last) != 0;
      }
      if (past) break;   // (wave-uniform: every used tile behind starts higher still)
   }
   if (lane < 2u) plan->end[lane] = zh_rg_find(src, S, tiles, lane ? t_last : t_lo, lane ? last : lo);
}

// One lane per tile of [t0, t1], striding: item (member - m0) of every member of [m0, m1]. A member with lo <= out_off and out_off + ISIZE <= hi goes to
// range_at + out_off - lo; m0 where it is not such a member to head_at, m1 to tail_at: its whole output, in the edge buffer. The three are offsets from ONE
// base address, the lower of the range's destination and the edge buffer, which the three launches take for their `dst`.
__global__ void __launch_bounds__(ZH_RG_THREADS)
zh_rg_items(const uint8_t *src, uint64_t S, const zh_ix_tile_t *__restrict__ tiles, uint64_t t0, uint64_t t1, uint64_t m0, uint64_t m1, uint64_t lo, uint64_t hi, uint64_t range_at,
            uint64_t head_at, uint64_t tail_at, zh_inflate_item_t *__restrict__ items) {
   for (uint64_t k = t0 + (uint64_t)blockIdx.x * ZH_RG_THREADS + threadIdx.x; k <= t1; k += (uint64_t)gridDim.x * ZH_RG_THREADS) {
      const zh_ix_tile_t r = tiles[k];
      if (!r.used || !r.members || r.member_base > m1 || r.member_base + r.members <= m0) continue;
      uint64_t p = r.entry, sum = r.out_base;
      for (uint32_t i = 0; i < r.members; i++) {
         const uint64_t m = r.member_base + i;
         if (m > m1) break;
         const zh_ix_walk_t w = zh_ix_walk<zh_ix_gzip_t, false>(src, S, p, p + 1u, NULL, 0);   // one hop
         if (w.stop != ZH_IX_MEMBER) break;
         if (m >= m0) {
            zh_inflate_item_t it;
            it.src_off = p;
            it.src_size = w.exit - p;
            it.dst_off = (sum >= lo && sum + w.out_sum <= hi) ? range_at + (sum - lo) : m == m0 ? head_at : tail_at;
            it.dst_cap = w.out_sum;
            items[m - m0] = it;
         }
         sum += w.out_sum;
         p = w.exit;
      }
   }
}

// `size` bytes from buf + at to d, of the slices the wave takes y, y + yslices, ...: zh_uz_copy's split into an interior of whole 16-byte chunks of the
// destination's address range and two bytewise edges. buf[0 .. B): what the aligned loads may touch.
__device__ __forceinline__ void zh_rg_move(const uint8_t *buf, uint64_t B, uint64_t at, uint8_t *d, uint64_t size, uint32_t y, uint32_t yslices, uint32_t lane) {
   const uintptr_t mask = ~(uintptr_t)15;
   const uint8_t *s = buf + at;
   const uintptr_t d0 = (uintptr_t)d, d1 = d0 + size;
   uintptr_t a0 = min((d0 + 15) & mask, d1), a1 = max(d1 & mask, a0);   // the interior [a0, a1); the edges [d0, a0) and [a1, d1)
   const uint32_t reach = ((uintptr_t)(s + (a0 - d0)) & 15u) ? 32u : 16u;
   if (a0 < a1 && ((uintptr_t)(s + (a0 - d0)) & mask) < (uintptr_t)buf) a0 += 16;
   if (a0 < a1 && ((uintptr_t)(s + (a1 - 16 - d0)) & mask) + reach > (uintptr_t)buf + B) a1 -= 16;
   if (y == 0) {
      for (uintptr_t q = d0 + lane; q < a0; q += 64) *(uint8_t *)q = s[q - d0];
      for (uintptr_t q = a1 + lane; q < d1; q += 64) *(uint8_t *)q = s[q - d0];
   }
   zh_copy_chunks((uint8_t *)a0, s + (a0 - d0), (uint32_t)((a1 - a0) >> 4), y, yslices, lane);
}

// One wave per workgroup; workgroup g works on edge g / yslices, slices g % yslices, + yslices, ... results: what zh_check_members has left of the batch.
__global__ void __launch_bounds__(ZH_RG_THREADS)
zh_rg_edges(const uint8_t *__restrict__ buf, uint64_t B, uint8_t *dst, zh_rg_edge_t head, zh_rg_edge_t tail, const zh_member_result_t *__restrict__ results, uint32_t yslices) {
   const uint32_t j = blockIdx.x / yslices, y = blockIdx.x % yslices;
   if (j > 1u) return;
   const zh_rg_edge_t e = j ? tail : head;
   if (e.to <= e.from) return;
   const uint64_t have = results[e.slot].out_size, to = have < e.to ? have : e.to;   // (a member that failed: what it has decoded of its slice)
   if (to <= e.from) return;
   zh_rg_move(buf, B, e.buf_at + e.from, dst + e.dst_at, to - e.from, y, yslices, zh_lane());   // (below 2^32 bytes: an ISIZE)
}
#endif
