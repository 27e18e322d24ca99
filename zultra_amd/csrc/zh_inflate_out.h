// zh_inflate_out.h — batched inflate: many independent raw deflate streams (RFC 1951), one wave64 each, the bytes written out.
//
// zh_verify.h checks a stream against the input it was made from; these kernels have no input to look at. The decoder is the same one,
// zh_deflate_dec.h's (bit reader, tables, block loop: what zlib's inflate accepts and rejects), over one item of the caller's source buffer
// (zh_d_item_src_t), in the inflate order of its verdicts; this file (names zh_i_) is its sink, zh_i_sink_t — the output path — and the kernels:
//
//   literals   one per lane per 64-byte stretch of the item's output, stored coalesced when the position leaves the stretch or a match needs them;
//   matches    lane l < len stores out[p + l] = out[p - dist + l % dist]: every source lies below p, so the (at most five) rounds of a match do
//              not depend on each other and dist < len needs no special case. The bytes a match reads were stored by OTHER lanes of this wave:
//              a workgroup-scope release / acquire (zh_wave_sync) and a drain of the wave's memory counter (zh_stores_done) stand between those
//              stores and the loads. They are issued only where the match's source reaches into bytes stored since the last time (`synced`):
//              far matches of a text run without them;
//   stored     a 64-lane byte copy from the stream, four loads in flight.
//
// The dictionary form (zh_i_sink_t<true>, zh_inflate_streams_dict) puts up to 32768 bytes of read-only history in front of every item's output:
// a source index below zero is taken from hist_end[index] instead of out[index], lane by lane, so one match may read both and may wrap while it
// still starts in the history. Nobody stores to the history during the launch: those loads need no release / acquire and no drain, and `synced` is
// compared, in signed arithmetic, with the end of the part of the source that lies in the output. <false> is the decoder without any of this.
//
// A stream may start at any byte address: the bit reader's base is that address aligned down to a dword and the first bit 8 * (address & 3). No
// byte outside the caller's source buffer is loaded (the two edge dwords of the buffer are put together from bytes), and bytes behind the ITEM's
// own end read as zero: a decode that wants them ends with ZH_V_STREAM_END, and the end of the item is looked at before every other verdict.
//
// The decoder is total: any byte string gives a verdict and nothing else. Every loop advances the bit position (bounded by the item's end) or
// the output position (bounded by dst_cap), every table index is masked, every store is checked against dst_cap (room()) and every match source
// against the item's own output start, or the history's (reach()), before it is issued. Runs of empty blocks are legal (zlib's sync flushes write
// them): the source size bounds them.
//
// One stream runs at the speed of one wave; the throughput of a batch is the number of waves resident (no scratch, ~3.4 KB of LDS per wave).
#pragma once
#include <stdint.h>

#include "zh_deflate_dec.h"

#define ZH_I_DST_FULL 13u   // the output does not fit in dst_cap (the reasons before it: zh_verify_reason)

// zultra_hip_inflate_item_t / zultra_hip_inflate_result_t (include/zultra_hip.h)
typedef struct zh_inflate_item_s {
   uint64_t src_off, src_size, dst_off, dst_cap;
} zh_inflate_item_t;
typedef struct zh_inflate_result_s {
   uint32_t reason, blocks;
   uint64_t out_size, src_used;
} zh_inflate_result_t;

#if defined(__HIPCC__) || defined(ZH_EMU)

// The sink of one stream: out[0 .. cap). DICT: hist_end[-hist_len .. 0) is what lies in front of out[0] for the matches (hist_len <= ZH_MAX_DIST);
// without it the two are not looked at.
template <bool DICT>
struct zh_i_sink_t {
   static constexpr uint32_t full = ZH_I_DST_FULL;
   uint8_t *out;
   uint64_t cap;
   const uint8_t *hist_end;
   uint32_t hist_len;
   uint32_t blocks;
   uint64_t p;        // bytes of output so far
   uint64_t synced;   // out[0 .. synced) was stored before the last release / acquire: any lane may load it
   uint32_t lit_val;
   uint64_t lit_group;
   bool lit_set;   // this lane holds the literal of position lit_group * 64 + lane

   __device__ __forceinline__ uint64_t room() const { return cap - p; }
   __device__ __forceinline__ uint64_t reach() const { return DICT ? p + hist_len : p; }   // (the start of the item's output, or of the history)
   // the pending literals of stretch lit_group of the item's output (all below cap: room() was asked when they were taken)
   __device__ __forceinline__ void flush() {
      if (lit_set) out[(lit_group << 6) + zh_lane()] = (uint8_t)lit_val;
      lit_set = false;
   }
   __device__ __forceinline__ void literal(uint32_t v) {
      if ((p >> 6) != lit_group) flush();   // p has left the stretch the lanes hold literals of
      lit_group = p >> 6;
      if (zh_lane() == ((uint32_t)p & 63u)) {
         lit_val = v;
         lit_set = true;
      }
      p++;
   }
   __device__ __forceinline__ void match(uint32_t len, uint32_t dist) {
      const uint32_t lane = zh_lane();
      flush();
      const bool wraps = dist < len;
      if (DICT) {
         // the source is [from, from + min(dist, len)), from >= -hist_len: what of it lies below zero is history, which nobody stores to
         const int64_t from = (int64_t)p - (int64_t)dist;
         const uint8_t *const hist = hist_end, *const o = out;   // (read here: a select between the two MEMBERS would keep the sink in memory)
         if (from + (int64_t)(wraps ? dist : len) > (int64_t)synced) {   // its part in the output reaches into bytes stored since the last release / acquire
            zh_wave_sync();
            zh_stores_done();
            synced = p;
         }
         for (uint32_t l = lane; l < len; l += 64u) {
            const int64_t i = from + (int64_t)(wraps ? l % dist : l);
            out[p + l] = i < 0 ? hist[i] : o[i];
         }
      }
      else {
         const uint64_t from = p - dist;
         if (from + (wraps ? dist : len) > synced) {   // the source reaches into bytes stored since the last release / acquire
            zh_wave_sync();
            zh_stores_done();   // (for a workgroup of one wave the compiler folds the fences into nothing: the drain is asked for by name)
            synced = p;
         }
         for (uint32_t l = lane; l < len; l += 64u) out[p + l] = out[from + (wraps ? l % dist : l)];   // (len <= 258: five rounds at most)
      }
      p += len;
   }
   __device__ __forceinline__ void stored(const uint8_t *s8, uint32_t len) {
      uint8_t *d8 = out + p;
      uint32_t i = zh_lane();
      for (; i + 192u < len; i += 256u) {   // four loads in flight
         const uint8_t a0 = s8[i], a1 = s8[i + 64u], a2 = s8[i + 128u], a3 = s8[i + 192u];
         d8[i] = a0;
         d8[i + 64u] = a1;
         d8[i + 128u] = a2;
         d8[i + 192u] = a3;
      }
      for (; i < len; i += 64u) d8[i] = s8[i];
      p += len;
   }
   __device__ __forceinline__ uint32_t block_end(bool past, uint32_t bfinal, bool *last) {
      if (past) return ZH_V_STREAM_END;   // (a block whose last bits lie behind the item's end is not counted)
      blocks++;
      *last = bfinal != 0;
      return ZH_V_OK;
   }
};

// One stream: bytes [it_lo, s.it_hi) from the reader's base -> out[0 .. cap). Returns the reason (wave-uniform).
template <bool DICT>
__device__ __forceinline__ uint32_t zh_inflate_one(zh_d_lds_t &S, const zh_d_item_src_t s, uint64_t it_lo, uint8_t *out, uint64_t cap, const uint8_t *hist_end, uint32_t hist_len,
                                                   uint32_t *pblocks, uint64_t *pout, uint64_t *pused) {
   const uint64_t end_bit = s.it_hi * 8u;
   *pblocks = 0;
   *pout = 0;
   *pused = 0;
   if (it_lo >= s.it_hi) return ZH_V_STREAM_END;
   zh_i_sink_t<DICT> K;
   K.out = out;
   K.cap = cap;
   K.hist_end = hist_end;
   K.hist_len = hist_len;
   K.blocks = 0;
   K.p = K.synced = 0;
   K.lit_val = 0;
   K.lit_group = 0;
   K.lit_set = false;
   zh_d_bits_t b;
   zh_d_seek(b, s, it_lo * 8u);
   const uint32_t reason = zh_d_blocks(S, b, s, end_bit, K);
   K.flush();
   *pblocks = K.blocks;
   *pout = K.p;
   const uint64_t at = zh_d_pos(b) < end_bit ? zh_d_pos(b) : end_bit;
   *pused = ((at + 7u) >> 3) - it_lo;
   return reason;
}

// One wave per stream, striding: the grid needs no count.
// (149 VGPRs as the compiler allots them: three waves to a SIMD, twelve streams to a CU. Held to 128 with amdgpu_waves_per_eu(4) the kernel spills 8 bytes
// to scratch memory, which no kernel here does.)
#define ZH_INFLATE_THREADS 64
template <bool DICT>
__device__ __forceinline__ void zh_inflate_items(zh_d_lds_t &S, const uint8_t *src, uint64_t src_size, uint8_t *dst, uint64_t dst_size, const uint8_t *hist_end, uint32_t hist_len,
                                                 const zh_inflate_item_t *__restrict__ items, uint32_t n, zh_inflate_result_t *__restrict__ results) {
   const uint64_t lead = (uint64_t)((uintptr_t)src & 3u);
   const uint32_t *base = (const uint32_t *)(src - lead);
   for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
      const zh_inflate_item_t it = items[k];
      zh_inflate_result_t r;
      r.reason = ZH_V_STREAM_END;
      r.blocks = 0;
      r.out_size = r.src_used = 0;
      if (it.dst_off > dst_size || it.dst_cap > dst_size - it.dst_off)   // (the host has refused such items: nothing is touched for them)
         r.reason = ZH_I_DST_FULL;
      else if (it.src_off <= src_size && it.src_size <= src_size - it.src_off) {
         zh_d_item_src_t s;
         s.base = base;
         s.buf_lo = lead;
         s.buf_hi = lead + src_size;
         s.it_hi = lead + it.src_off + it.src_size;
         r.reason = zh_inflate_one<DICT>(S, s, lead + it.src_off, dst + it.dst_off, it.dst_cap, hist_end, hist_len, &r.blocks, &r.out_size, &r.src_used);
      }
      if (zh_lane() == 0) results[k] = r;
      zh_sync();   // (the tables in LDS are the next stream's)
   }
}
__global__ void __launch_bounds__(ZH_INFLATE_THREADS)
zh_inflate_streams(const uint8_t *src, uint64_t src_size, uint8_t *dst, uint64_t dst_size, const zh_inflate_item_t *__restrict__ items, uint32_t n, zh_inflate_result_t *__restrict__ results) {
   __shared__ zh_d_lds_t S;
   zh_inflate_items<false>(S, src, src_size, dst, dst_size, NULL, 0, items, n, results);
}
// ... with one preset dictionary for every item: hist_end is the byte behind its last one (any byte address), hist_len <= 32768 of them are history.
__global__ void __launch_bounds__(ZH_INFLATE_THREADS)
zh_inflate_streams_dict(const uint8_t *src, uint64_t src_size, uint8_t *dst, uint64_t dst_size, const uint8_t *hist_end, uint32_t hist_len, const zh_inflate_item_t *__restrict__ items, uint32_t n,
                        zh_inflate_result_t *__restrict__ results) {
   __shared__ zh_d_lds_t S;
   zh_inflate_items<true>(S, src, src_size, dst, dst_size, hist_end, hist_len < ZH_MAX_DIST ? hist_len : ZH_MAX_DIST, items, n, results);
}
#endif
