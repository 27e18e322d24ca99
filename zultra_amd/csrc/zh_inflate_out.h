// zh_inflate_out.h — batched inflate: many independent raw deflate streams (RFC 1951), one wave64 each, the bytes written out.
//
// zh_inflate.h checks a stream against the input it was made from; this kernel has no input to look at. It shares that decoder's bit reader
// state (zh_v_bits_t), its table builder and symbol decode (zh_v_build, zh_v_sym: what zlib's inflate accepts and rejects) and its LDS layout,
// and adds the output path:
//
//   literals   one per lane per 64-byte stretch of the item's output, stored coalesced when the position leaves the stretch or a match needs them;
//   matches    lane l < len stores out[p + l] = out[p - dist + l % dist]: every source lies below p, so the (at most five) rounds of a match do
//              not depend on each other and dist < len needs no special case. The bytes a match reads were stored by OTHER lanes of this wave:
//              a workgroup-scope release / acquire (zh_wave_sync) and a drain of the wave's memory counter (zh_stores_done) stand between those
//              stores and the loads. They are issued only where the match's source reaches into bytes stored since the last time (`synced`):
//              far matches of a text run without them;
//   stored     a 64-lane byte copy from the stream, four loads in flight.
//
// The dictionary form (zh_inflate_one<true>, zh_inflate_streams_dict) puts up to 32768 bytes of read-only history in front of every item's output:
// a source index below zero is taken from hist_end[index] instead of out[index], lane by lane, so one match may read both and may wrap while it
// still starts in the history. Nobody stores to the history during the launch: those loads need no release / acquire and no drain, and `synced` is
// compared, in signed arithmetic, with the end of the part of the source that lies in the output. <false> is the decoder without any of this.
//
// A stream may start at any byte address: the bit reader's base is that address aligned down to a dword and the first bit 8 * (address & 3). No
// byte outside the caller's source buffer is loaded (the two edge dwords of the buffer are put together from bytes), and bytes behind the ITEM's
// own end read as zero: a decode that wants them ends with ZH_V_STREAM_END.
//
// The decoder is total: any byte string gives a verdict and nothing else. Every loop advances the bit position (bounded by the item's end) or
// the output position (bounded by dst_cap), every table index is masked, every store is checked against dst_cap and every match source against
// the item's own output start before it is issued. Runs of empty blocks are legal (zlib's sync flushes write them): the source size bounds them.
//
// One stream runs at the speed of one wave; the throughput of a batch is the number of waves resident (no scratch, ~3.4 KB of LDS per wave).
#pragma once
#include <stdint.h>

#include "zh_inflate.h"

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

// byte offsets from the bit reader's base (the source buffer's address aligned down to a dword)
struct zh_i_src_t {
   uint64_t buf_lo, buf_hi;   // the caller's whole source buffer
   uint64_t it_hi;            // end of the item
};
__device__ __forceinline__ void zh_i_window(zh_v_bits_t &b, const zh_i_src_t &s) {
   const uint64_t lo = (b.next_dw + zh_lane()) * 4u;
   uint32_t w = 0;
   if (lo < s.it_hi) {
      if (lo >= s.buf_lo && lo + 4u <= s.buf_hi)
         w = b.stream[lo >> 2];
      else {   // (the buffer starts or ends inside this dword)
         const uint8_t *s8 = (const uint8_t *)b.stream;
         for (uint32_t k = 0; k < 4u; k++)
            if (lo + k >= s.buf_lo && lo + k < s.buf_hi) w |= (uint32_t)s8[lo + k] << (8u * k);
      }
      if (lo + 4u > s.it_hi) w &= (1u << (8u * (uint32_t)(s.it_hi - lo))) - 1u;   // (1..3 bytes of the item in it)
   }
   b.w = w;
   b.widx = 0;
}
__device__ __forceinline__ void zh_i_fill(zh_v_bits_t &b, const zh_i_src_t &s) {
   if (b.have <= 32u) {
      if (b.widx >= 64u) zh_i_window(b, s);
      b.hold |= (uint64_t)zh_readlane(b.w, (int)(b.widx & 63u)) << b.have;
      b.have += 32u;
      b.widx++;
      b.next_dw++;
   }
}
__device__ __forceinline__ void zh_i_seek(zh_v_bits_t &b, const zh_i_src_t &s, uint64_t bit) {
   b.next_dw = bit >> 5;
   zh_i_window(b, s);
   b.hold = 0;
   b.have = 0;
   zh_i_fill(b, s);
   const uint32_t r = (uint32_t)bit & 31u;
   b.hold >>= r;
   b.have -= r;
}
__device__ __forceinline__ uint32_t zh_i_get(zh_v_bits_t &b, const zh_i_src_t &s, uint32_t n) {
   zh_i_fill(b, s);
   return zh_v_take(b, n);
}

// the pending literals of stretch `group` of the item's output (all below dst_cap: checked when they were taken)
__device__ __forceinline__ void zh_i_flush(uint8_t *out, uint64_t group, uint32_t lit_val, bool &lit_set) {
   if (lit_set) out[(group << 6) + zh_lane()] = (uint8_t)lit_val;
   lit_set = false;
}

// The code lengths of a dynamic block (RFC 1951 3.2.7) into S.lens: the parse of zh_verify_one, with the end of the item looked at before every
// other verdict (a cut-off stream is ZH_V_STREAM_END, whatever the zero bits behind its end would decode to).
__device__ __forceinline__ uint32_t zh_i_dynamic_lens(zh_v_lds_t &S, zh_v_bits_t &b, const zh_i_src_t &s, uint64_t end_bit, uint32_t *pnlit, uint32_t *pndist) {
   const uint32_t lane = zh_lane();
   const uint32_t nlit = zh_i_get(b, s, 5) + 257u;
   const uint32_t ndist = zh_i_get(b, s, 5) + 1u;
   const uint32_t ncl = zh_i_get(b, s, 4) + 4u;
   if (zh_v_pos(b) > end_bit) return ZH_V_STREAM_END;
   if (nlit > 286u || ndist > 30u) return ZH_V_HEADER;
   if (lane < 19u) S.lens[lane] = 0;
   zh_sync();
   for (uint32_t i = 0; i < ncl; i++) {
      const uint32_t v = zh_i_get(b, s, 3);
      if (lane == 0) S.lens[zh_v_cl_order[i]] = (uint8_t)v;
   }
   if (zh_v_pos(b) > end_bit) return ZH_V_STREAM_END;
   zh_sync();
   if (zh_v_build(S.lens, 19, S.cl, ZH_V_CL_BITS, S.sorted_dist, 31u, S.cnt[1], S.next, S.offs, true) != 0) return ZH_V_CODELENS;
   const uint32_t n = nlit + ndist;   // (both alphabets as one run-length coded sequence: a run may cross from the literals into the distances)
   uint32_t i = 0, prev = 0;
   while (i < n) {
      zh_i_fill(b, s);
      const int sym = zh_v_sym(b, S.cl, ZH_V_CL_BITS, S.sorted_dist, 31u, S.cnt[1]);
      if (sym < 0) return zh_v_pos(b) + 15u > end_bit ? ZH_V_STREAM_END : ZH_V_CODELENS;
      uint32_t rep = 1, val = (uint32_t)sym;
      if (sym == 16) {
         val = prev;
         rep = 3u + zh_v_take(b, 2);
      }
      else if (sym == 17) {
         val = 0;
         rep = 3u + zh_v_take(b, 3);
      }
      else if (sym >= 18) {
         val = 0;
         rep = 11u + zh_v_take(b, 7);
      }
      if (zh_v_pos(b) > end_bit) return ZH_V_STREAM_END;
      if (sym > 18 || (sym == 16 && i == 0) || i + rep > n) return ZH_V_CODELENS;
      for (uint32_t j = lane; j < rep; j += 64u) S.lens[(i + j) & 511u] = (uint8_t)val;   // (i + j < n <= 316: the mask is the rule, not a need)
      prev = val;
      i += rep;
   }
   zh_sync();
   if (S.lens[256] == 0) return ZH_V_CODELENS;   // no end-of-block code
   *pnlit = nlit;
   *pndist = ndist;
   return ZH_V_OK;
}

// One stream: bytes [it_lo, it_hi) from the reader's base -> out[0 .. cap). Returns the reason (wave-uniform).
// DICT: hist_end[-hist_len .. 0) is what lies in front of out[0] for the matches (hist_len <= ZH_MAX_DIST); without it the two are not looked at.
template <bool DICT>
__device__ __forceinline__ uint32_t zh_inflate_one(zh_v_lds_t &S, const uint32_t *base, const zh_i_src_t s, uint64_t it_lo, uint8_t *out, uint64_t cap, const uint8_t *hist_end, uint32_t hist_len,
                                                   uint32_t *pblocks, uint64_t *pout, uint64_t *pused) {
   const uint32_t lane = zh_lane();
   const uint64_t end_bit = s.it_hi * 8u;
   zh_v_bits_t b;
   b.stream = base;
   b.ndw = (s.it_hi + 3u) >> 2;
   uint32_t reason = ZH_V_OK, blocks = 0;
   uint64_t p = 0;        // bytes of output so far
   uint64_t synced = 0;   // out[0 .. synced) was stored before the last release / acquire: any lane may load it
   uint32_t lit_val = 0;
   uint64_t lit_group = 0;
   bool lit_set = false;   // this lane holds the literal of position lit_group * 64 + lane
   *pblocks = 0;
   *pout = 0;
   *pused = 0;
   if (it_lo >= s.it_hi) return ZH_V_STREAM_END;
   zh_i_seek(b, s, it_lo * 8u);

   for (;;) {
      if (zh_v_pos(b) + 3u > end_bit) {
         reason = ZH_V_STREAM_END;
         break;
      }
      const uint32_t hdr = zh_i_get(b, s, 3);
      const uint32_t bfinal = hdr & 1u, btype = hdr >> 1;
      if (btype == 3u) {
         reason = ZH_V_HEADER;
         break;
      }
      if (btype == 0u) {
         // stored: LEN and NLEN on the next byte boundary (the pad bits are ignored, RFC 1951 3.2.4), then LEN bytes
         const uint64_t byte = (zh_v_pos(b) + 7u) >> 3;
         if (byte + 4u > s.it_hi) {
            reason = ZH_V_STREAM_END;
            break;
         }
         zh_i_seek(b, s, byte * 8u);
         const uint32_t len = zh_i_get(b, s, 16), nlen = zh_i_get(b, s, 16);
         if (len != (~nlen & 0xffffu))
            reason = ZH_V_STORED_LEN;
         else if (byte + 4u + len > s.it_hi)
            reason = ZH_V_STREAM_END;
         else if (len > cap - p)
            reason = ZH_I_DST_FULL;
         if (reason != ZH_V_OK) break;
         const uint8_t *s8 = (const uint8_t *)base + byte + 4u;
         uint8_t *d8 = out + p;
         uint32_t i = lane;
         for (; i + 192u < len; i += 256u) {   // four loads in flight
            const uint8_t a0 = s8[i], a1 = s8[i + 64u], a2 = s8[i + 128u], a3 = s8[i + 192u];
            d8[i] = a0;
            d8[i + 64u] = a1;
            d8[i + 128u] = a2;
            d8[i + 192u] = a3;
         }
         for (; i < len; i += 64u) d8[i] = s8[i];
         p += len;
         if (len) zh_i_seek(b, s, (byte + 4u + len) * 8u);
      }
      else {
         uint32_t nlit = 288, ndist = 32;
         if (btype == 1u) {
            for (uint32_t i = lane; i < 320u; i += 64u) S.lens[i] = (uint8_t)(i < 288u ? zh_static_lit_len((int)i) : 5);
            zh_sync();
         }
         else {
            reason = zh_i_dynamic_lens(S, b, s, end_bit, &nlit, &ndist);
            if (reason != ZH_V_OK) break;
         }
         if (zh_v_build(S.lens, nlit, S.lit, ZH_V_LIT_BITS, S.sorted_lit, 511u, S.cnt[0], S.next, S.offs, false) != 0 ||
             zh_v_build(S.lens + nlit, ndist, S.dist, ZH_V_DIST_BITS, S.sorted_dist, 31u, S.cnt[1], S.next, S.offs, false) != 0) {
            reason = ZH_V_CODELENS;
            break;
         }
         // ---- tokens
         for (;;) {
            zh_i_fill(b, s);
            const int sym = zh_v_sym(b, S.lit, ZH_V_LIT_BITS, S.sorted_lit, 511u, S.cnt[0]);
            if (sym < 0) {
               reason = zh_v_pos(b) + 15u > end_bit ? ZH_V_STREAM_END : ZH_V_SYMBOL;
               break;
            }
            if (sym < 256) {
               if (zh_v_pos(b) > end_bit) {
                  reason = ZH_V_STREAM_END;
                  break;
               }
               if (p >= cap) {
                  reason = ZH_I_DST_FULL;
                  break;
               }
               if ((p >> 6) != lit_group) zh_i_flush(out, lit_group, lit_val, lit_set);   // p has left the stretch the lanes hold literals of
               lit_group = p >> 6;
               if (lane == ((uint32_t)p & 63u)) {
                  lit_val = (uint32_t)sym;
                  lit_set = true;
               }
               p++;
               continue;
            }
            if (sym == ZH_EOB) break;   // (its bits are looked at behind the block)
            uint32_t len = 0, dist = 0;
            int ds = 0;
            if (sym < 286) {
               const int li = sym - 257;
               len = zh_lenidx_base(li) + zh_v_take(b, (uint32_t)zh_lenidx_xbits(li));
               zh_i_fill(b, s);
               ds = zh_v_sym(b, S.dist, ZH_V_DIST_BITS, S.sorted_dist, 31u, S.cnt[1]);
               if (ds >= 0 && ds < 30) dist = zh_dist_base(ds) + zh_v_take(b, (uint32_t)zh_dist_xbits(ds));
            }
            if (zh_v_pos(b) + (ds < 0 ? 15u : 0u) > end_bit)
               reason = ZH_V_STREAM_END;
            else if (sym >= 286)
               reason = ZH_V_SYMBOL;
            else if (ds < 0 || ds >= 30 || dist > ZH_MAX_DIST || dist > (DICT ? p + hist_len : p))   // (it reaches in front of the item's output, or of the history)
               reason = ZH_V_DISTANCE;
            else if (len > cap - p)
               reason = ZH_I_DST_FULL;
            if (reason != ZH_V_OK) break;
            zh_i_flush(out, lit_group, lit_val, lit_set);
            const bool wraps = dist < len;
            if (DICT) {
               // the source is [from, from + min(dist, len)), from >= -hist_len: what of it lies below zero is history, which nobody stores to
               const int64_t from = (int64_t)p - (int64_t)dist;
               if (from + (int64_t)(wraps ? dist : len) > (int64_t)synced) {   // its part in the output reaches into bytes stored since the last release / acquire
                  zh_wave_sync();
                  zh_stores_done();
                  synced = p;
               }
               for (uint32_t l = lane; l < len; l += 64u) {
                  const int64_t i = from + (int64_t)(wraps ? l % dist : l);
                  out[p + l] = i < 0 ? hist_end[i] : out[i];
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
         if (reason != ZH_V_OK) break;
      }
      if (zh_v_pos(b) > end_bit) {
         reason = ZH_V_STREAM_END;
         break;
      }
      blocks++;
      if (bfinal) break;
   }
   zh_i_flush(out, lit_group, lit_val, lit_set);
   *pblocks = blocks;
   *pout = p;
   const uint64_t at = zh_v_pos(b) < end_bit ? zh_v_pos(b) : end_bit;
   *pused = ((at + 7u) >> 3) - it_lo;
   return reason;
}

// One wave per stream, striding: the grid needs no count.
// (149 VGPRs as the compiler allots them: three waves to a SIMD, twelve streams to a CU. Held to 128 with amdgpu_waves_per_eu(4) the kernel spills 8 bytes
// to scratch memory, which no kernel here does.)
#define ZH_INFLATE_THREADS 64
template <bool DICT>
__device__ __forceinline__ void zh_inflate_items(zh_v_lds_t &S, const uint8_t *src, uint64_t src_size, uint8_t *dst, uint64_t dst_size, const uint8_t *hist_end, uint32_t hist_len,
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
         zh_i_src_t s;
         s.buf_lo = lead;
         s.buf_hi = lead + src_size;
         s.it_hi = lead + it.src_off + it.src_size;
         r.reason = zh_inflate_one<DICT>(S, base, s, lead + it.src_off, dst + it.dst_off, it.dst_cap, hist_end, hist_len, &r.blocks, &r.out_size, &r.src_used);
      }
      if (zh_lane() == 0) results[k] = r;
      zh_sync();   // (the tables in LDS are the next stream's)
   }
}
__global__ void __launch_bounds__(ZH_INFLATE_THREADS)
zh_inflate_streams(const uint8_t *src, uint64_t src_size, uint8_t *dst, uint64_t dst_size, const zh_inflate_item_t *__restrict__ items, uint32_t n, zh_inflate_result_t *__restrict__ results) {
   __shared__ zh_v_lds_t S;
   zh_inflate_items<false>(S, src, src_size, dst, dst_size, NULL, 0, items, n, results);
}
// ... with one preset dictionary for every item: hist_end is the byte behind its last one (any byte address), hist_len <= 32768 of them are history.
__global__ void __launch_bounds__(ZH_INFLATE_THREADS)
zh_inflate_streams_dict(const uint8_t *src, uint64_t src_size, uint8_t *dst, uint64_t dst_size, const uint8_t *hist_end, uint32_t hist_len, const zh_inflate_item_t *__restrict__ items, uint32_t n,
                        zh_inflate_result_t *__restrict__ results) {
   __shared__ zh_v_lds_t S;
   zh_inflate_items<true>(S, src, src_size, dst, dst_size, hist_end, hist_len < ZH_MAX_DIST ? hist_len : ZH_MAX_DIST, items, n, results);
}
#endif
