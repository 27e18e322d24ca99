// zh_streams.h — the GROUPED assembly: a batch that holds several deflate streams, each a run of consecutive max-blocks.
//
// Between the two layouts zh_stitch_scan knows — one stream that carries its bit phase across all max-blocks, and every max-block a byte-aligned stream of its
// own — lies the one a batch of large inputs needs: inside a stream the phase is carried and the history is real, between streams there is a BFINAL and a
// byte-aligned restart. stream_of[b] (one word per max-block, uploaded with the call) = the stream of max-block b, with ZH_STREAM_START where b is its first.
//
//   zh_stitch_scan_streams  one workgroup, the transfer-table scan of zh_stitch_scan: a chunk of max-blocks is a map (bit & 7 at its entry) -> bits it adds, WITH
//                           the alignments, heads and tails of the streams that start and end inside it — they round the running bit up to a byte and add a
//                           constant, so what a chunk adds still depends on nothing but the phase at its entry, and the tables compose as in stream mode;
//   zh_fold_streams         one wave per stream: size, CRC-32 linear part and Adler sums of the stream from those of its max-blocks (zh_crc32_blocks), in the shape
//                           the writers read per max-block — so zh_frame_members, zh_zip_scan, zh_zip_records and zh_zip_copy run over streams as they are.
// zh_stitch_plan_streams (zh_stitch.h) is the host's statement of the rule, which the tests hold the scan to.
#pragma once
#include "zh_frame.h"

#if defined(__HIPCC__) || defined(ZH_EMU)

// The items, file_off[0 .. nstreams] and the report of a grouped assembly. head / tail: bytes left free in front of and behind every stream (zh_frame.h); member s is
// bytes file_off[s] - head .. file_off[s + 1] - head, end_bit the end of the last tail. The start phase is 0; table_end is not meaningful here and reads 0.
__global__ void __launch_bounds__(ZH_SCAN_THREADS)
zh_stitch_scan_streams(const zh_subblock_t *__restrict__ subs, const uint32_t *__restrict__ nsubs_p, uint32_t nblocks, uint32_t nstreams, uint32_t max_block_size, uint32_t head, uint32_t tail,
                       const uint32_t *__restrict__ stream_of, uint32_t *blk_start /* scratch, nblocks + 1 */, zh_stitch_item_t *items, uint64_t *file_off /* nstreams + 1 */, zh_scan_out_t *out) {
   __shared__ uint32_t T[ZH_SCAN_THREADS][8];      // per chunk and phase at its entry: bits added
   __shared__ uint64_t Wv[ZH_SCAN_THREADS / 64][8];                                // the same per wave of chunks
   __shared__ uint64_t wave_start[ZH_SCAN_THREADS / 64 + 1];
   __shared__ uint64_t chunk_start[ZH_SCAN_THREADS];
   __shared__ uint32_t s_failed;
   const uint32_t tid = threadIdx.x;
   const uint32_t nsubs = *nsubs_p;
   if (nsubs == 0xFFFFFFFFu) {   // (a void run in the batch, zh_compact_results: nothing to assemble)
      if (tid == 0) {
         out->end_bit = 0;
         out->failed = 1;
         out->nsubs = nsubs;
         out->table_failed = 0xffu;
         out->oversize = 0;
      }
      return;
   }
   const uint64_t cap = zh_stitch_blockbuf_cap(max_block_size);
   const uint64_t head_bits = 8ull * head, tail_bits = 8ull * tail;
   if (tid == 0) s_failed = 0;
   // ---- 0: where every max-block's sub-blocks start
   for (uint32_t k = tid; k < nsubs; k += ZH_SCAN_THREADS)
      if (k == 0 || subs[k].block != subs[k - 1].block) blk_start[subs[k].block] = k;
   if (tid == 0) blk_start[nblocks] = nsubs;
   __threadfence_block();
   __syncthreads();
   const uint32_t per = (nblocks + ZH_SCAN_THREADS - 1) / ZH_SCAN_THREADS;
   const uint32_t B0 = min(nblocks, tid * per), B1 = min(nblocks, B0 + per);
   // ---- 1: the chunk's table. A chunk may begin in the middle of a stream: entry phase q is a start at bit q
   {
      uint64_t bit[8], base[8];
#pragma unroll
      for (uint32_t p = 0; p < 8; p++) bit[p] = p;
      for (uint32_t b = B0; b < B1; b++) {
         const uint32_t k0 = blk_start[b], k1 = blk_start[b + 1];
         const bool starts = (stream_of[b] & ZH_STREAM_START) != 0, ends = b + 1 == nblocks || (stream_of[b + 1] & ZH_STREAM_START) != 0;
#pragma unroll
         for (uint32_t p = 0; p < 8; p++) {
            if (starts) bit[p] = ((bit[p] + 7) & ~7ull) + head_bits;
            base[p] = bit[p] >> 3;
         }
         for (uint32_t k = k0; k < k1; k++) {
            const uint32_t size = subs[k].size, failed = subs[k].failed;
            const uint64_t nbits = subs[k].nbits;
#pragma unroll
            for (uint32_t p = 0; p < 8; p++) {
               uint32_t stored;
               (void)zh_stitch_step(&bit[p], base[p], size, nbits, failed, cap, &stored);   // (an overflow: step 3 meets it on the true walk, and nothing is written)
            }
         }
         if (ends) {
#pragma unroll
            for (uint32_t p = 0; p < 8; p++) bit[p] = ((bit[p] + 7) & ~7ull) + tail_bits;
         }
      }
#pragma unroll
      for (uint32_t p = 0; p < 8; p++) T[tid][p] = (uint32_t)(bit[p] - p);
   }
   __syncthreads();
   // ---- 2a: per wave of chunks and entry phase
   if (tid < (ZH_SCAN_THREADS / 64) * 8) {
      const uint32_t w = tid >> 3, p = tid & 7;
      uint64_t bit = p;
      for (uint32_t c = w * 64; c < w * 64 + 64; c++) bit += T[c][bit & 7];
      Wv[w][p] = bit - p;
   }
   __syncthreads();
   // ---- 2b: the waves from phase 0
   if (tid == 0) {
      uint64_t bit = 0;
      for (uint32_t w = 0; w < ZH_SCAN_THREADS / 64; w++) {
         wave_start[w] = bit;
         bit += Wv[w][bit & 7];
      }
      wave_start[ZH_SCAN_THREADS / 64] = bit;
   }
   __syncthreads();
   // ---- 2c: the chunks of every wave from the wave's true start
   if ((tid & 63u) == 0) {
      const uint32_t w = tid >> 6;
      uint64_t bit = wave_start[w];
      for (uint32_t c = w * 64; c < w * 64 + 64; c++) {
         chunk_start[c] = bit;
         bit += T[c][bit & 7];
      }
   }
   __syncthreads();
   // ---- 3: the items, and the streams' first bytes
   {
      uint64_t bit = chunk_start[tid];
      uint32_t fail = 0;
      for (uint32_t b = B0; b < B1; b++) {
         const uint32_t k0 = blk_start[b], k1 = blk_start[b + 1], so = stream_of[b];
         const bool ends = b + 1 == nblocks || (stream_of[b + 1] & ZH_STREAM_START) != 0;
         if (so & ZH_STREAM_START) {
            bit = ((bit + 7) & ~7ull) + head_bits;
            file_off[so & ~ZH_STREAM_START] = bit >> 3;
         }
         const uint64_t base = bit >> 3;
         for (uint32_t k = k0; k < k1; k++) {
            zh_stitch_item_t it;
            it.dst_bit = bit;
            it.is_final = (k + 1 == k1 && ends) ? 1u : 0u;
            it.stored = 0;
            if (zh_stitch_step(&bit, base, subs[k].size, subs[k].nbits, subs[k].failed, cap, &it.stored) != 0) fail = 1;
            items[k] = it;
         }
         if (ends) bit = ((bit + 7) & ~7ull) + tail_bits;
      }
      if (fail) atomicOr(&s_failed, 1u);
   }
   __syncthreads();
   if (tid == 0) {
      const uint64_t end = wave_start[ZH_SCAN_THREADS / 64];   // (behind the last stream's tail: a whole byte)
      file_off[nstreams] = (end >> 3) + head;
      out->end_bit = end;
      out->failed = s_failed;
      out->table_failed = 0;
      out->oversize = 0;
      out->nsubs = nsubs;
      for (uint32_t p = 0; p < 8; p++) out->table_end[p] = 0;
   }
}

// ---- the streams' sizes and checksums from their max-blocks' -------------------------------------------------------------------------------------------------
// What is known of a run of bytes: its length, its CRC-32 linear part (zero initial state, no final inversion), its Adler sums A = sum of the bytes and
// Bw = sum of (n - i) * byte[i], both mod 65521 (zh_crc32_blocks). Runs join: lin(A || B) = lin(A) * x^(8 |B|) + lin(B) over GF(2) mod P;
// A = A_A + A_B, Bw = Bw_A + |B| * A_A + Bw_B. The empty run {0, 0, 0, 0} is the identity, and the operation is associative.
struct zh_fold_t {
   uint64_t n;
   uint32_t crc, a, bw;
};
__device__ __forceinline__ uint32_t zh_gf2_x8n(uint64_t n) {   // x^(8n) mod P: square-and-multiply over the bits of n
   uint32_t q = 0x80000000u >> 8, p = 0x80000000u;
   for (uint64_t m = n; m; m >>= 1) {
      if (m & 1u) p = zh_gf2_mulmod(q, p);
      q = zh_gf2_mulmod(q, q);
   }
   return p;
}
__device__ __forceinline__ zh_fold_t zh_fold_join(const zh_fold_t L, const zh_fold_t R) {
   zh_fold_t J;
   J.n = L.n + R.n;
   J.crc = zh_gf2_mulmod(L.crc, zh_gf2_x8n(R.n)) ^ R.crc;
   J.a = (L.a + R.a) % ZH_ADLER_MOD;
   J.bw = (uint32_t)(((uint64_t)L.bw + (R.n % ZH_ADLER_MOD) * L.a + R.bw) % ZH_ADLER_MOD);
   return J;
}

// One wave per stream, striding. Lane l folds a contiguous sub-run of the stream's max-blocks — streams are few and long: one lane per stream would fold a whole
// batch serially —, the 64 partial results are joined pairwise in LDS, in order. stream_first[s] .. stream_first[s + 1] - 1 are the stream's max-blocks
// (stream_first[nstreams] = the batch's block count). Out, per stream, what the writers read per max-block: sblocks[s] = {the stream's first byte, no history, its
// size}, scrc[s], sadler[2s], sadler[2s + 1]. A size of 2^32 or more does not fit n: the host, which knows the sizes, refuses such a grouping before it launches.
#define ZH_FOLD_THREADS 64
__global__ void __launch_bounds__(ZH_FOLD_THREADS)
zh_fold_streams(const zh_block_t *__restrict__ blocks, const uint32_t *__restrict__ crc, const uint32_t *__restrict__ adler, const uint32_t *__restrict__ stream_first, uint32_t nstreams,
                zh_block_t *sblocks, uint32_t *scrc, uint32_t *sadler) {
   __shared__ zh_fold_t part[ZH_FOLD_THREADS];
   const uint32_t lane = threadIdx.x;
   for (uint32_t s = blockIdx.x; s < nstreams; s += gridDim.x) {
      const uint32_t b0 = stream_first[s], b1 = stream_first[s + 1], nb = b1 - b0;
      const uint32_t per = (nb + ZH_FOLD_THREADS - 1) / ZH_FOLD_THREADS;
      const uint32_t lo = b0 + min(nb, lane * per), hi = min(b1, lo + per);
      zh_fold_t acc = {0, 0, 0, 0};
      for (uint32_t b = lo; b < hi; b++) {
         const zh_fold_t r = {blocks[b].n, crc[b], adler[2 * b], adler[2 * b + 1]};
         acc = zh_fold_join(acc, r);
      }
      part[lane] = acc;
      for (uint32_t d = 1; d < ZH_FOLD_THREADS; d <<= 1) {   // part[l] covers lanes l .. l + 2d - 1 after the step
         zh_sync();
         if ((lane & (2 * d - 1)) == 0) part[lane] = zh_fold_join(part[lane], part[lane + d]);
      }
      if (lane == 0) {
         zh_block_t sb;
         sb.win_off = blocks[b0].win_off + blocks[b0].prev;
         sb.prev = 0;
         sb.n = (uint32_t)part[0].n;
         sblocks[s] = sb;
         scrc[s] = part[0].crc;
         sadler[2 * s] = part[0].a;
         sadler[2 * s + 1] = part[0].bw;
      }
      zh_sync();   // (part is the next stream's)
   }
}
#endif
