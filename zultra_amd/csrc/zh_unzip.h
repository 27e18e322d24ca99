// zh_unzip.h — a ZIP archive read on the device: the central directory indexed, the local headers checked against it, deflated entries
// inflated by zh_inflate_out.h's kernel, stored ones copied, and every entry's CRC-32 taken and compared by zh_check_members' ZIP form.
//
// The DIRECTORY is src[D0 .. D1). A RECORD starts at p when D1 - p >= 46, src[p..p+4) = 50 4b 01 02 and, with n, m, k the le16 values at p + 28, p + 30 and
// p + 32 (name, extra field, comment), p + 46 + n + m + k <= D1; the next position is p + 46 + n + m + k. The INDEX is the chain from D0; it stops with a kind:
// 0 p == D1; 1 fewer than 46 bytes left, or no signature; 2 a record that runs past D1. The chain is serial — a million records are a million dependent loads
// —, so it is walked as zh_inflate_index.h walks gzip members: speculated per tile of T bytes, verified, the rare miss walked again. The three passes are that
// header's, with the format below; every result equals the serial walk bit for bit for any bytes in src.
//
//   zh_uz_tiles    one wave per tile: the first position in the tile that starts a record (the four signature bytes: three may lie behind a lane's window),
//                  then one lane hops from that guess to the tile's end and stores the tile record
//   zh_uz_resolve  one lane: the chain of tiles from D0; a tile whose guess is not the chain's entry is walked again (tiles_rewalked)
//   zh_uz_entries  one lane per tile the chain entered: a 48-byte zh_zip_dirent_t per record, dst_off the 64-bit sum of the `size` fields in front of it
//   zh_uz_locals   one lane per entry, from the dirent alone: 17 (a method other than 0 and 8; flag bit 0, 5 or 6; a 0xFFFFFFFF size or offset); else the local
//                  header at local_off + local_delta: 14 where its 30 bytes do not lie in src, the signature, the name (length and bytes) or the method differ
//                  from the central record's, the data runs past the source, or a stored entry has comp_size != size. The local header's sizes and CRC, a data
//                  descriptor and a ZIP64 extra field there are not looked at: the central record is the authority. Out: the inflate kernel's item for a deflated
//                  entry (an empty one for the others), an entry of the copy list for a stored one, the preliminary result.
//   zh_uz_copy     the stored entries, source to destination at independent byte addresses: zh_copy.h's mover, a wave per entry and slice
#pragma once
#include <stdint.h>

#include "zh_copy.h"
#include "zh_inflate_check.h"
#include "zh_inflate_index.h"

#define ZH_UZ_TILE (16u * 1024u)   // bytes of the directory per tile, where ZULTRA_HIP_INDEX_TILE does not say: measured (profiles/unzip_time.txt)
#define ZH_UZ_CENTRAL 46u
#define ZH_UZ_LOCAL 30u
#define ZH_UZ_THREADS 64
#define ZH_UZ_COPY_THREADS 256
#define ZH_UZ_MAX_YSLICES 32u

struct zh_uz_copy_t {   // a stored entry: `size` bytes from src + src_at to dst + dst_at
   uint64_t src_at, dst_at, size;
};

#if defined(__HIPCC__) || defined(ZH_EMU)

__device__ __forceinline__ uint32_t zh_uz_le32(const uint8_t *q) { return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24); }

// The central directory as a record format of zh_inflate_index.h's walk: the value summed is `size`.
struct zh_uz_format_t {
   typedef zh_zip_dirent_t item_t;
   static constexpr uint32_t SIG = 0x02014b50u, SIG_MASK = 0xFFFFFFFFu, BEHIND = 3u;
   static __device__ __forceinline__ uint32_t probe(const uint8_t *src, uint64_t D1, uint64_t p, uint32_t *len, uint32_t *val) {
      if (p == D1) return 0u;
      const uint8_t *q = src + p;
      if (D1 - p < ZH_UZ_CENTRAL || zh_uz_le32(q) != SIG) return 1u;
      const uint32_t L = ZH_UZ_CENTRAL + zh_ix_le16(q + 28) + zh_ix_le16(q + 30) + zh_ix_le16(q + 32);
      if ((uint64_t)L > D1 - p) return 2u;
      *len = L;
      *val = zh_uz_le32(q + 24);
      return ZH_IX_MEMBER;
   }
   static __device__ __forceinline__ void put(zh_zip_dirent_t *item, const uint8_t *src, uint64_t p, uint32_t len, uint64_t sum, uint32_t val) {
      const uint8_t *q = src + p;
      zh_zip_dirent_t e;
      e.central_at = p;
      e.local_off = zh_uz_le32(q + 42);
      e.dst_off = sum;
      e.comp_size = zh_uz_le32(q + 20);
      e.size = val;
      e.crc32 = zh_uz_le32(q + 16);
      e.name_len = zh_ix_le16(q + 28);
      e.method = (uint16_t)zh_ix_le16(q + 10);
      e.flags = (uint16_t)zh_ix_le16(q + 8);
      e.extra_len = (uint16_t)zh_ix_le16(q + 30);
      e.comment_len = (uint16_t)zh_ix_le16(q + 32);
      *item = e;
   }
};

__global__ void __launch_bounds__(ZH_IX_THREADS)
zh_uz_tiles(const uint8_t *src, uint64_t S, uint64_t D0, uint64_t D1, uint64_t T, uint64_t ntiles, zh_ix_tile_t *__restrict__ tiles) {
   zh_ix_tiles_pass<zh_uz_format_t>(src, S, D0, D1, T, ntiles, tiles);
}
__global__ void __launch_bounds__(ZH_IX_THREADS)
zh_uz_resolve(const uint8_t *src, uint64_t D0, uint64_t D1, uint64_t T, uint64_t ntiles, zh_ix_tile_t *tiles, zh_ix_totals_t *totals) {
   zh_ix_resolve_pass<zh_uz_format_t>(src, D0, D1, T, ntiles, tiles, totals);
}
__global__ void __launch_bounds__(ZH_IX_THREADS)
zh_uz_entries(const uint8_t *src, uint64_t D0, uint64_t D1, uint64_t T, uint64_t ntiles, const zh_ix_tile_t *__restrict__ tiles, zh_zip_dirent_t *__restrict__ dirents) {
   zh_ix_items_pass<zh_uz_format_t>(src, D0, D1, T, ntiles, tiles, dirents);
}

// One lane per entry, striding. local_delta: what turns a central record's offset into a position in src (the host keeps it within +-2^62).
// ncopies: zeroed by the host; copies has room for every entry.
__global__ void __launch_bounds__(ZH_UZ_THREADS)
zh_uz_locals(const uint8_t *src, uint64_t S, const zh_zip_dirent_t *__restrict__ dirents, uint32_t n, int64_t local_delta, zh_inflate_item_t *__restrict__ inner,
             zh_member_result_t *__restrict__ results, zh_uz_copy_t *copies, uint32_t *ncopies) {
   for (uint64_t i = (uint64_t)blockIdx.x * ZH_UZ_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * ZH_UZ_THREADS) {
      const zh_zip_dirent_t e = dirents[i];
      uint32_t reason = 0, head = 0;
      uint64_t data_at = 0;
      if ((e.method != 0 && e.method != 8) || (e.flags & 0x61u) || e.comp_size == 0xFFFFFFFFu || e.size == 0xFFFFFFFFu || e.local_off == 0xFFFFFFFFull)
         reason = ZH_M_UNSUPPORTED;
      else {
         reason = ZH_M_BAD_FRAME;
         const int64_t lp = (int64_t)e.local_off + local_delta;
         if (lp >= 0 && (uint64_t)lp <= S && S - (uint64_t)lp >= ZH_UZ_LOCAL) {
            const uint8_t *q = src + lp;
            const uint32_t n_local = zh_ix_le16(q + 26), m_local = zh_ix_le16(q + 28);
            head = ZH_UZ_LOCAL + n_local + m_local;
            data_at = (uint64_t)lp + head;
            bool ok = zh_uz_le32(q) == 0x04034b50u && n_local == e.name_len && zh_ix_le16(q + 8) == e.method && data_at <= S && e.comp_size <= S - data_at &&
                      (e.method != 0 || e.comp_size == e.size);
            if (ok) {   // (the local name lies in front of data_at, the central one inside the directory: both in src)
               const uint8_t *name = src + e.central_at + ZH_UZ_CENTRAL;
               for (uint32_t k = 0; k < n_local && ok; k++) ok = q[ZH_UZ_LOCAL + k] == name[k];
            }
            if (ok) reason = 0;
         }
      }
      zh_inflate_item_t in;
      in.src_off = in.src_size = in.dst_off = in.dst_cap = 0;   // (nothing is decoded or written for it: the inflate kernel ends it with reason 12, which nobody reads)
      if (!reason && e.method == 8) {
         in.src_off = data_at;
         in.src_size = e.comp_size;
         in.dst_off = e.dst_off;
         in.dst_cap = e.size;
      }
      inner[i] = in;
      if (!reason && e.method == 0 && e.size) {
         zh_uz_copy_t c;
         c.src_at = data_at;
         c.dst_at = e.dst_off;
         c.size = e.size;
         copies[zh_atomic_add_global(ncopies, 1u)] = c;
      }
      zh_member_result_t r;
      r.reason = reason;
      r.blocks = 0;
      r.out_size = r.src_used = 0;
      r.head_size = reason ? 0u : head;
      r.check = 0;
      results[i] = r;
   }
}

// The copy list. Work is (entry, slice) as in zh_zip_copy: a wave takes an entry, of ZH_UZ_COPY_THREADS / 64 per workgroup, and of it the slices y, y + yslices, ...;
// workgroup g is x = g / yslices along the list and y = g % yslices along the slices. The interior — the 16-byte chunks of the destination's ADDRESS range that lie
// wholly inside the entry — goes through zh_copy_chunks, whose aligned loads reach up to 15 bytes in front of the data and up to 15 behind it: in front lie the 30
// bytes of the local header at least; behind, the last chunk is left to the bytewise edge where its loads would pass the end of src. No load outside src[0 .. S).
__global__ void __launch_bounds__(ZH_UZ_COPY_THREADS)
zh_uz_copy(const uint8_t *__restrict__ src, uint64_t S, uint8_t *dst, const zh_uz_copy_t *__restrict__ copies, const uint32_t *__restrict__ ncopies, uint32_t yslices) {
   const uint32_t n = *ncopies, lane = threadIdx.x & 63u, waves = blockDim.x >> 6;
   const uint32_t y = blockIdx.x % yslices, x = blockIdx.x / yslices, xdim = gridDim.x / yslices;
   const uintptr_t mask = ~(uintptr_t)15;
   for (uint32_t e = x * waves + (threadIdx.x >> 6); e < n; e += xdim * waves) {
      const zh_uz_copy_t c = copies[e];
      const uint8_t *s = src + c.src_at;   // the source of d0
      const uintptr_t d0 = (uintptr_t)(dst + c.dst_at), d1 = d0 + c.size;
      uintptr_t a0 = min((d0 + 15) & mask, d1), a1 = max(d1 & mask, a0);   // the interior [a0, a1); the edges [d0, a0) and [a1, d1)
      const uint32_t reach = ((uintptr_t)(s + (a0 - d0)) & 15u) ? 32u : 16u;   // what a chunk's loads cover, from its first source byte's address aligned down
      if (a0 < a1 && ((uintptr_t)(s + (a0 - d0)) & mask) < (uintptr_t)src) a0 += 16;   // (never, with a local header in front)
      if (a0 < a1 && ((uintptr_t)(s + (a1 - 16 - d0)) & mask) + reach > (uintptr_t)src + S) a1 -= 16;   // (one chunk back is enough: its loads end at most where the data does)
      if (y == 0) {
         for (uintptr_t d = d0 + lane; d < a0; d += 64) *(uint8_t *)d = s[d - d0];
         for (uintptr_t d = a1 + lane; d < d1; d += 64) *(uint8_t *)d = s[d - d0];
      }
      zh_copy_chunks((uint8_t *)a0, s + (a0 - d0), (uint32_t)((a1 - a0) >> 4), y, yslices, lane);
   }
}
#endif
