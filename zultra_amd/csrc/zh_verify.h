// zh_verify.h — verification: inflate every sub-block of the last stitched batch on the device and compare it with the batch's input.
//
// The stream buffer holds the finished deflate stream, the context still holds the input windows, and the stitch left for every sub-block
// its first header bit (zh_stitch_item_t.dst_bit) and its input range (zh_subblock_t). With the ORIGINAL input at hand a sub-block is checked
// without any other: a literal at input position p is right when it equals in[p], a match (len, dist) at p exactly when
// in[p .. p+len) == in[p-dist .. p-dist+len) — no decoded history is needed. By induction over the stream this is what a serial inflater
// produces, given that every sub-block's decode ends exactly where the next one starts and that BFINAL appears only where it should
// (DESIGN.md 3.8). The decoder is zh_deflate_dec.h's — written from RFC 1951, accepting what zlib's inflate accepts — over the whole stream
// buffer (zh_d_stream_src_t), in the verify order of its verdicts; this file (names zh_v_) is its sink, zh_v_sink_t, and the kernel.
//
//   zh_verify_subblocks  one wave64 per sub-block, striding. The decode state (bit position, input position) is wave-uniform, the decode tables
//                        are built in LDS by the wave, ~4 KB. The lanes do the comparing: no compare result feeds the decode — mismatches are
//                        kept per lane and looked at once per deflate block, and the bytes a compare loads are only looked at when the next
//                        compare is issued, so that their latency stays off the serial chain.
//
// The decoder is total: any byte string in the stream buffer gives a verdict and nothing else. Every bit read is bounded by the stream's
// end (dwords behind it read as zero, and the position is checked once per token), every table index is masked, every input index is
// checked against the item's window before the load (room() and reach() in front of every literal, match and stored run), every loop advances
// the bit position or the input position, both bounded (a run of blocks without a byte: max_empty).
#pragma once
#include <stdint.h>

#include "zh_common.h"
#include "zh_deflate_dec.h"
#include "zh_stitch.h"

// per sub-block: what the wave found
typedef struct zh_verify_item_s {
   uint32_t reason;
   uint32_t block;
   uint64_t input_off;    // offset inside the max-block
   uint64_t stream_bit;   // where the decoder stood
} zh_verify_item_t;

// per batch (32-bit words: the atomics the emulator has)
typedef struct zh_verify_report_s {
   uint32_t bad;           // sub-blocks that did not verify
   uint32_t first_bad;     // the first of them in stream order, 0xFFFFFFFF if none
   uint32_t verified_lo, verified_hi;   // input bytes of the sub-blocks that verified
} zh_verify_report_t;

#if defined(__HIPCC__) || defined(ZH_EMU)
// ---- the lanes' compares: issued now, looked at when the next one is issued ------------------------------------------------------------
struct zh_v_cmp_t {
   uint32_t a, b, pos, kind;     // the compare in flight
   uint32_t bad_at, bad_kind;    // this lane's first mismatch of the block so far (input position inside the sub-block), 0xFFFFFFFF: none
};
__device__ __forceinline__ void zh_v_cmp_settle(zh_v_cmp_t &c) {
   if (c.a != c.b && c.pos < c.bad_at) {
      c.bad_at = c.pos;
      c.bad_kind = c.kind;
   }
   c.a = c.b = 0;
}

// The sink of one sub-block: in[0 .. size) is what it has to decode to, `back` bytes of the window lie in front of in[0].
struct zh_v_sink_t {
   static constexpr uint32_t full = ZH_V_SIZE;
   const uint8_t *in;
   uint32_t back, size, is_final;
   uint32_t p, p0, nempty;   // input position; where the block began; blocks without a byte so far
   zh_v_cmp_t cmp;
   uint32_t lit_val, lit_group;
   bool lit_set, lit_any;   // lit_set: this lane holds the literal of position lit_group * 64 + lane; lit_any: some lane does

   __device__ __forceinline__ uint32_t room() const { return size - p; }
   __device__ __forceinline__ uint32_t reach() const { return back + p; }
   // the literals the lanes hold against the input, one coalesced load
   __device__ __forceinline__ void literals_out() {
      zh_v_cmp_settle(cmp);
      if (lit_set) {
         cmp.a = in[(lit_group << 6) + zh_lane()];
         cmp.b = lit_val;
         cmp.pos = (lit_group << 6) + zh_lane();
         cmp.kind = ZH_V_LITERAL;
      }
      lit_set = false;
   }
   __device__ __forceinline__ void literal(uint32_t v) {
      if (lit_any && (p >> 6) != lit_group) literals_out();   // p has left the 64-byte stretch the lanes hold literals of
      lit_group = p >> 6;
      lit_any = true;
      if (zh_lane() == (p & 63u)) {
         lit_val = v;
         lit_set = true;
      }
      p++;
   }
   __device__ __forceinline__ void match(uint32_t len, uint32_t dist) {
      for (uint32_t l = zh_lane(); l < len; l += 64u) {   // (len <= 258: five rounds at most; the lanes of a round wait for the round before)
         zh_v_cmp_settle(cmp);
         cmp.a = in[p + l];
         cmp.b = in[(int64_t)(p + l) - (int64_t)dist];
         cmp.pos = p + l;
         cmp.kind = ZH_V_MATCH;
      }
      p += len;
   }
   __device__ __forceinline__ void stored(const uint8_t *s8, uint32_t len) {
      const uint8_t *d8 = in + p;
      uint32_t i = zh_lane();
      for (; i + 192u < len; i += 256u) {   // four loads of each side in flight
         const uint32_t a0 = s8[i], a1 = s8[i + 64u], a2 = s8[i + 128u], a3 = s8[i + 192u];
         const uint32_t b0 = d8[i], b1 = d8[i + 64u], b2 = d8[i + 128u], b3 = d8[i + 192u];
         const uint32_t at = a0 != b0 ? i : a1 != b1 ? i + 64u : a2 != b2 ? i + 128u : i + 192u;
         if ((a0 != b0 || a1 != b1 || a2 != b2 || a3 != b3) && p + at < cmp.bad_at) {
            cmp.bad_at = p + at;
            cmp.bad_kind = ZH_V_STORED_BYTES;
         }
      }
      for (; i < len; i += 64u)
         if (s8[i] != d8[i] && p + i < cmp.bad_at) {
            cmp.bad_at = p + i;
            cmp.bad_kind = ZH_V_STORED_BYTES;
         }
      p += len;
   }
   // The block is decoded: now what the compares found, and only then the end of the stream, BFINAL and the run of empty blocks.
   __device__ __forceinline__ uint32_t block_end(bool past, uint32_t bfinal, bool *last) {
      if (lit_any) literals_out();
      lit_any = false;
      zh_v_cmp_settle(cmp);
      if (zh_ballot(cmp.bad_at != 0xFFFFFFFFu) != 0) {
         const uint32_t at = zh_wave_min(cmp.bad_at);
         const int who = zh_ctz64(zh_ballot(cmp.bad_at == at));
         p = at;   // (the report's position: nothing is decoded behind a mismatch)
         return zh_readlane(cmp.bad_kind, who & 63);
      }
      if (past) return ZH_V_STREAM_END;
      if (bfinal != ((is_final && p == size) ? 1u : 0u)) return ZH_V_BFINAL;
      *last = p == size;
      if (p == p0 && !*last && ++nempty > size / 65535u + 2u) return ZH_V_HEADER;
      p0 = p;
      return ZH_V_OK;
   }
};

// One sub-block. Returns the reason (wave-uniform); *err_pos = input position inside the sub-block, *err_bit = stream bit.
__device__ __forceinline__ uint32_t zh_verify_one(zh_d_lds_t &S, const uint32_t *__restrict__ stream, uint64_t end_bit, const zh_stitch_item_t it, const uint8_t *__restrict__ in, uint32_t back,
                                                  uint32_t size, uint32_t *err_pos, uint64_t *err_bit) {
   *err_pos = 0;
   *err_bit = it.dst_bit;
   if (it.dst_bit >= end_bit) return ZH_V_STREAM_END;
   zh_d_stream_src_t s;
   s.base = stream;
   s.ndw = (end_bit + 31u) >> 5;
   zh_v_sink_t K;
   K.in = in;
   K.back = back;
   K.size = size;
   K.is_final = it.is_final;
   K.p = K.p0 = K.nempty = 0;
   K.cmp.a = K.cmp.b = K.cmp.pos = K.cmp.kind = 0;
   K.cmp.bad_at = 0xFFFFFFFFu;
   K.cmp.bad_kind = 0;
   K.lit_val = K.lit_group = 0;
   K.lit_set = K.lit_any = false;
   zh_d_bits_t b;
   zh_d_seek(b, s, it.dst_bit);
   const uint32_t reason = zh_d_blocks(S, b, s, end_bit, K);
   *err_pos = K.p;
   *err_bit = zh_d_pos(b);
   return reason;
}

// One wave per sub-block of the last stitched batch, striding: the grid needs no count. files != 0: the batch was stitched as one stream per
// max-block (zh_stitch_scan): a max-block's last sub-block ends within the last byte before the next file's first — or, where the assembly left `gap` bytes
// of trailer and header between the streams (zh_frame.h; file_off[nblocks] counts a gap as well), that many bytes earlier.
// files == 2: the grouped form (zh_streams.h) — stream_of[b] = the stream of max-block b, ZH_STREAM_START where b starts it, and file_off is indexed by stream:
// the sub-block that ends a stream's last max-block ends like a file's, every other sub-block where the next one begins.
#define ZH_VERIFY_THREADS 64
#ifdef ZH_EMU
#define ZH_VERIFY_WAVES_PER_SIMD
#else
#define ZH_VERIFY_WAVES_PER_SIMD __attribute__((amdgpu_waves_per_eu(3)))   // at most 168 VGPRs: a CU then holds twelve sub-blocks, the chip 3072 (the chains are serial: residency is the throughput)
#endif
__global__ void __launch_bounds__(ZH_VERIFY_THREADS) ZH_VERIFY_WAVES_PER_SIMD
zh_verify_subblocks(const uint32_t *__restrict__ stream, uint64_t stream_cap, const zh_stitch_item_t *__restrict__ items, const zh_subblock_t *__restrict__ subs,
                    const zh_block_t *__restrict__ blocks, uint32_t nblocks, const uint8_t *__restrict__ data, const zh_scan_out_t *__restrict__ scan, const uint64_t *__restrict__ file_off,
                    int files, uint32_t gap, const uint32_t *__restrict__ stream_of /* files == 2 */, zh_verify_item_t *out, zh_verify_report_t *report) {
   __shared__ zh_d_lds_t S;
   if (scan->failed) return;   // (nothing was stitched: the host does not ask then)
   const uint32_t nsubs = scan->nsubs;
   const uint64_t end_bit = scan->end_bit < stream_cap * 8u ? scan->end_bit : stream_cap * 8u;
   for (uint32_t k = blockIdx.x; k < nsubs; k += gridDim.x) {
      const zh_subblock_t sb = subs[k];
      const zh_stitch_item_t it = items[k];
      uint32_t reason, err_pos = 0;
      uint64_t err_bit = it.dst_bit;
      if (sb.block >= nblocks)
         reason = ZH_V_SIZE;
      else {
         const zh_block_t blk = blocks[sb.block];
         if ((uint64_t)sb.start + sb.size > blk.n)
            reason = ZH_V_SIZE;
         else {
            reason = zh_verify_one(S, stream, end_bit, it, data + blk.win_off + blk.prev + sb.start, blk.prev + sb.start, sb.size, &err_pos, &err_bit);
            if (reason == ZH_V_OK) {
               const bool last_of_block = k + 1u == nsubs || subs[k + 1u].block != sb.block;
               const bool last_of_stream = last_of_block && (files == 1 || (files == 2 && (sb.block + 1u == nblocks || (stream_of[sb.block + 1u] & ZH_STREAM_START))));
               const uint32_t next = files == 2 ? (stream_of[sb.block] & ~ZH_STREAM_START) + 1u : sb.block + 1u;   // (what follows in file_off)
               const bool ends = last_of_stream ? ((err_bit + 7u) >> 3) + gap == file_off[next] : err_bit == (k + 1u < nsubs ? items[k + 1u].dst_bit : end_bit);
               if (!ends) reason = ZH_V_END_BIT;
            }
         }
      }
      if (zh_lane() == 0) {
         zh_verify_item_t r;
         r.reason = reason;
         r.block = sb.block;
         r.input_off = (uint64_t)sb.start + err_pos;
         r.stream_bit = err_bit;
         out[k] = r;
         if (reason != ZH_V_OK) {
            atomicAdd(&report->bad, 1u);
            atomicMin(&report->first_bad, k);
         }
         else {
            const uint32_t old = atomicAdd(&report->verified_lo, sb.size);
            if (old > 0xFFFFFFFFu - sb.size) atomicAdd(&report->verified_hi, 1u);
         }
      }
      zh_sync();   // (the tables in LDS are the next sub-block's)
   }
}
#endif
