// zh_inflate.h — verification: inflate every sub-block of the last stitched batch on the device and compare it with the batch's input.
//
// The stream buffer holds the finished deflate stream, the context still holds the input windows, and the stitch left for every sub-block
// its first header bit (zh_stitch_item_t.dst_bit) and its input range (zh_subblock_t). With the ORIGINAL input at hand a sub-block is checked
// without any other: a literal at input position p is right when it equals in[p], a match (len, dist) at p exactly when
// in[p .. p+len) == in[p-dist .. p-dist+len) — no decoded history is needed. By induction over the stream this is what a serial inflater
// produces, given that every sub-block's decode ends exactly where the next one starts and that BFINAL appears only where it should
// (DESIGN.md 3.8). The decoder is written from RFC 1951; what it accepts is what zlib's inflate accepts (over-subscribed and incomplete
// code sets are rejected, except the incomplete set of a single one-bit code; HLIT > 286 and HDIST > 30 are rejected).
//
//   zh_verify_subblocks  one wave64 per sub-block, striding. The decode state (bit position, input position) is wave-uniform; the bits come
//                        from a window of 64 dwords held one per lane (loaded coalesced, read with zh_readlane), the decode tables (a 9-bit
//                        primary table for literals / lengths, 8-bit for distances, a canonical length-count walk behind both) are built in
//                        LDS by the wave, ~4 KB. The lanes do the comparing: no compare result feeds the decode — mismatches are kept per
//                        lane and looked at once per deflate block, and the bytes a compare loads are only looked at when the next compare
//                        is issued, so that their latency stays off the serial chain.
//
// The decoder is total: any byte string in the stream buffer gives a verdict and nothing else. Every bit read is bounded by the stream's
// end (dwords behind it read as zero, and the position is checked once per token), every table index is masked, every input index is
// checked against the item's window before the load, every loop advances the bit position or the input position, both bounded.
#pragma once
#include <stdint.h>

#include "zh_common.h"
#include "zh_stitch.h"

// reasons (include/zultra_hip.h: ZULTRA_HIP_VERIFY_OK and the list behind it)
enum zh_verify_reason {
   ZH_V_OK = 0,
   ZH_V_HEADER = 1,        // BTYPE 3, HLIT / HDIST out of range, a run of empty blocks
   ZH_V_CODELENS = 2,      // code length code or code lengths: over-subscribed, incomplete, bad repeat, no end-of-block code
   ZH_V_SYMBOL = 3,        // no such literal / length code, symbols 286 and 287
   ZH_V_DISTANCE = 4,      // no such distance code, symbols 30 and 31, a distance that reaches in front of the window
   ZH_V_LITERAL = 5,       // a literal differs from the input
   ZH_V_MATCH = 6,         // a match copies other bytes than the input has
   ZH_V_STORED_LEN = 7,    // LEN != ~NLEN
   ZH_V_STORED_BYTES = 8,  // stored bytes differ from the input
   ZH_V_SIZE = 9,          // the blocks decode to more bytes than the sub-block has (or the descriptor leaves its max-block)
   ZH_V_END_BIT = 10,      // the decode does not end where the next sub-block starts
   ZH_V_BFINAL = 11,       // BFINAL set where it should not be, or missing on the stream's last block
   ZH_V_STREAM_END = 12,   // the decode runs past the end of the stream
};

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
#include <zh_platform.h>

#define ZH_V_LIT_BITS 9u
#define ZH_V_DIST_BITS 8u
#define ZH_V_CL_BITS 7u
#define ZH_V_ENTRY(sym, len) ((uint16_t)((sym) | ((len) << 9)))   // symbol < 512, code length 1..15; 0 = no code of at most `bits` bits starts like this

struct zh_v_lds_t {
   uint16_t lit[1u << ZH_V_LIT_BITS];
   uint16_t dist[1u << ZH_V_DIST_BITS];
   uint16_t cl[1u << ZH_V_CL_BITS];
   uint16_t sorted_lit[512];   // symbols in (code length, symbol) order: the canonical walk's answer; 288 used, indexed & 511
   uint16_t sorted_dist[32];   // ... 32 used, indexed & 31 (also the code length code's while the lengths are read)
   uint32_t cnt[2][16];        // codes per length: [0] literals / lengths, [1] distances (and the code length code)
   uint32_t next[16], offs[16];   // builder: first code and first sorted slot of every length
   uint8_t lens[320];
};

static __device__ const uint8_t zh_v_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};   // RFC 1951 3.2.7

// ---- the bit reader: wave-uniform state, 64 dwords of the stream one per lane --------------------------------------------------------
struct zh_v_bits_t {
   const uint32_t *stream;
   uint64_t ndw;       // dwords that hold bits of the stream: behind them everything reads as zero
   uint64_t next_dw;   // the dword `hold` is refilled from next (the window covers next_dw - widx .. + 64)
   uint64_t hold;      // the next `have` bits, LSB first
   uint32_t have, widx;
   uint32_t w;         // per lane: dword (window start + lane)
};
__device__ __forceinline__ void zh_v_window(zh_v_bits_t &b) {
   const uint64_t i = b.next_dw + zh_lane();
   b.w = i < b.ndw ? b.stream[i] : 0u;
   b.widx = 0;
}
// at least 32 bits in hold afterwards (a literal / length code with its extra bits takes 20 at most, a distance 28)
__device__ __forceinline__ void zh_v_fill(zh_v_bits_t &b) {
   if (b.have <= 32u) {
      if (b.widx >= 64u) zh_v_window(b);
      b.hold |= (uint64_t)zh_readlane(b.w, (int)(b.widx & 63u)) << b.have;
      b.have += 32u;
      b.widx++;
      b.next_dw++;
   }
}
__device__ __forceinline__ uint64_t zh_v_pos(const zh_v_bits_t &b) { return (b.next_dw << 5) - b.have; }
__device__ __forceinline__ void zh_v_seek(zh_v_bits_t &b, uint64_t bit) {
   b.next_dw = bit >> 5;
   zh_v_window(b);
   b.hold = 0;
   b.have = 0;
   zh_v_fill(b);
   const uint32_t r = (uint32_t)bit & 31u;
   b.hold >>= r;
   b.have -= r;
}
// n <= 16 bits that are in hold (the caller has filled)
__device__ __forceinline__ uint32_t zh_v_take(zh_v_bits_t &b, uint32_t n) {
   const uint32_t v = (uint32_t)b.hold & ((1u << n) - 1u);
   b.hold >>= n;
   b.have -= n;
   return v;
}
__device__ __forceinline__ uint32_t zh_v_get(zh_v_bits_t &b, uint32_t n) {
   zh_v_fill(b);
   return zh_v_take(b, n);
}

// ---- decode tables of one alphabet ---------------------------------------------------------------------------------------------------
// lens[0 .. n) (values 0..15) -> primary table of 2^tbits entries, the symbols in canonical order, the counts per length. Wave-uniform result:
// 0 = usable (a set without any code included: every decode then fails), 1 = over-subscribed, 2 = incomplete — which zlib accepts only for a
// single code of one bit, and never for the code length code (is_cl).
__device__ __forceinline__ int zh_v_build(const uint8_t *lens, uint32_t n, uint16_t *table, uint32_t tbits, uint16_t *sorted, uint32_t smask, uint32_t *cnt, uint32_t *next,
                                          uint32_t *offs, bool is_cl) {
   const uint32_t lane = zh_lane();
   if (lane < 16u) cnt[lane] = 0;
   for (uint32_t i = lane; i < (1u << tbits); i += 64u) table[i] = 0;
   zh_sync();
   for (uint32_t i = lane; i < n; i += 64u) {
      const uint32_t L = lens[i] & 15u;
      if (L) atomicAdd(&cnt[L], 1u);
   }
   zh_sync();
   int left = 1;
   bool over = false;
   uint32_t code = 0, off = 0, maxlen = 0;
   for (uint32_t L = 1; L <= 15u; L++) {
      const uint32_t c = cnt[L];
      left = (left << 1) - (int)c;
      if (left < 0) {
         over = true;
         left = 0;
      }
      if (c) maxlen = L;
      if (lane == 0) {
         next[L] = code;
         offs[L] = off;
      }
      code = (code + c) << 1;
      off += c;
   }
   zh_sync();
   if (over) return 1;
   if (maxlen && left > 0 && (is_cl || maxlen != 1u)) return 2;
   // lane L assigns the codes of length L in symbol order (not over-subscribed: every code is below 2^L)
   if (lane >= 1u && lane <= 15u && cnt[lane]) {
      const uint32_t L = lane;
      uint32_t c = next[L], o = offs[L];
      for (uint32_t s = 0; s < n; s++) {
         if ((lens[s] & 15u) != L) continue;
         sorted[o & smask] = (uint16_t)s;
         o++;
         if (L <= tbits) {
            uint32_t r = 0, v = c;
            for (uint32_t q = 0; q < L; q++) {   // Huffman codes go into the stream from their most significant bit
               r = (r << 1) | (v & 1u);
               v >>= 1;
            }
            for (uint32_t j = r; j < (1u << tbits); j += 1u << L) table[j] = ZH_V_ENTRY(s, L);
         }
         c++;
      }
   }
   zh_sync();
   return 0;
}

// next symbol (hold has 15 bits or more, zero bits behind the stream's end), -1 where the bits are no code of the set
__device__ __forceinline__ int zh_v_sym(zh_v_bits_t &b, const uint16_t *table, uint32_t tbits, const uint16_t *sorted, uint32_t smask, const uint32_t *cnt) {
   const uint32_t e = table[(uint32_t)b.hold & ((1u << tbits) - 1u)];
   if (e >> 9) {
      b.hold >>= e >> 9;
      b.have -= e >> 9;
      return (int)(e & 511u);
   }
   // canonical walk, one bit per length: code - first is the code's rank among the codes of its length
   uint32_t code = 0, first = 0, index = 0;
   uint64_t h = b.hold;
   for (uint32_t L = 1; L <= 15u; L++) {
      code |= (uint32_t)h & 1u;
      h >>= 1;
      const uint32_t c = cnt[L];
      if (code >= first && code - first < c) {
         b.hold = h;
         b.have -= L;
         return (int)sorted[(index + (code - first)) & smask];
      }
      index += c;
      first = (first + c) << 1;
      code <<= 1;
   }
   return -1;
}

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

// One sub-block. Returns the reason (wave-uniform); *err_pos = input position inside the sub-block, *err_bit = stream bit.
__device__ __forceinline__ uint32_t zh_verify_one(zh_v_lds_t &S, const uint32_t *__restrict__ stream, uint64_t end_bit, const zh_stitch_item_t it, const uint8_t *__restrict__ in, uint32_t back,
                                                  uint32_t size, uint32_t *err_pos, uint64_t *err_bit) {
   const uint32_t lane = zh_lane();
   zh_v_bits_t b;
   b.stream = stream;
   b.ndw = (end_bit + 31u) >> 5;
   zh_v_cmp_t cmp;
   cmp.a = cmp.b = cmp.pos = cmp.kind = 0;
   cmp.bad_at = 0xFFFFFFFFu;
   cmp.bad_kind = 0;
   uint32_t reason = ZH_V_OK, p = 0, nempty = 0;
   const uint32_t max_empty = size / 65535u + 2u;
   *err_pos = 0;
   *err_bit = it.dst_bit;
   if (it.dst_bit >= end_bit) return ZH_V_STREAM_END;
   zh_v_seek(b, it.dst_bit);

   while (reason == ZH_V_OK) {
      const uint32_t p0 = p;
      if (zh_v_pos(b) + 3u > end_bit) {
         reason = ZH_V_STREAM_END;
         break;
      }
      const uint32_t hdr = zh_v_get(b, 3);
      const uint32_t bfinal = hdr & 1u, btype = hdr >> 1;
      if (btype == 3u)
         reason = ZH_V_HEADER;
      else if (btype == 0u) {
         // stored: LEN and NLEN on the next byte boundary (the pad bits are ignored, RFC 1951 3.2.4), then LEN bytes
         const uint64_t byte = (zh_v_pos(b) + 7u) >> 3;
         if ((byte + 4u) * 8u > end_bit) {
            reason = ZH_V_STREAM_END;
            break;
         }
         zh_v_seek(b, byte * 8u);
         const uint32_t len = zh_v_get(b, 16), nlen = zh_v_get(b, 16);
         if (len != (~nlen & 0xffffu))
            reason = ZH_V_STORED_LEN;
         else if (len > size - p)
            reason = ZH_V_SIZE;
         else if ((byte + 4u + len) * 8u > end_bit)
            reason = ZH_V_STREAM_END;
         else {
            const uint8_t *s8 = (const uint8_t *)stream + byte + 4u;
            const uint8_t *d8 = in + p;
            uint32_t i = lane;
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
            zh_v_seek(b, (byte + 4u + len) * 8u);
         }
      }
      else {
         // ---- the two alphabets' code lengths
         uint32_t nlit = 288, ndist = 32;
         if (btype == 1u) {
            for (uint32_t i = lane; i < 320u; i += 64u) S.lens[i] = (uint8_t)(i < 288u ? zh_static_lit_len((int)i) : 5);
            zh_sync();
         }
         else {
            nlit = zh_v_get(b, 5) + 257u;
            ndist = zh_v_get(b, 5) + 1u;
            const uint32_t ncl = zh_v_get(b, 4) + 4u;
            if (nlit > 286u || ndist > 30u) {
               reason = ZH_V_HEADER;
               break;
            }
            if (lane < 19u) S.lens[lane] = 0;
            zh_sync();
            for (uint32_t i = 0; i < ncl; i++) {
               const uint32_t v = zh_v_get(b, 3);
               if (lane == 0) S.lens[zh_v_cl_order[i]] = (uint8_t)v;
            }
            zh_sync();
            if (zh_v_build(S.lens, 19, S.cl, ZH_V_CL_BITS, S.sorted_dist, 31u, S.cnt[1], S.next, S.offs, true) != 0) {
               reason = ZH_V_CODELENS;
               break;
            }
            // the lengths of both alphabets as one run-length coded sequence: a run may cross from the literals into the distances
            const uint32_t n = nlit + ndist;
            uint32_t i = 0, prev = 0;
            while (i < n) {
               zh_v_fill(b);
               if (zh_v_pos(b) > end_bit) {
                  reason = ZH_V_STREAM_END;
                  break;
               }
               const int s = zh_v_sym(b, S.cl, ZH_V_CL_BITS, S.sorted_dist, 31u, S.cnt[1]);
               if (s < 0 || s > 18) {
                  reason = ZH_V_CODELENS;
                  break;
               }
               if (s < 16) {
                  if (lane == 0) S.lens[i] = (uint8_t)s;
                  prev = (uint32_t)s;
                  i++;
                  continue;
               }
               uint32_t rep, val = 0;
               if (s == 16) {
                  if (i == 0) {
                     reason = ZH_V_CODELENS;
                     break;
                  }
                  val = prev;
                  rep = 3u + zh_v_take(b, 2);
               }
               else if (s == 17)
                  rep = 3u + zh_v_take(b, 3);
               else
                  rep = 11u + zh_v_take(b, 7);
               if (i + rep > n) {
                  reason = ZH_V_CODELENS;
                  break;
               }
               for (uint32_t j = lane; j < rep; j += 64u) S.lens[i + j] = (uint8_t)val;
               prev = val;
               i += rep;
            }
            if (reason != ZH_V_OK) break;
            zh_sync();
            if (S.lens[256] == 0) {   // no end-of-block code
               reason = ZH_V_CODELENS;
               break;
            }
         }
         if (zh_v_build(S.lens, nlit, S.lit, ZH_V_LIT_BITS, S.sorted_lit, 511u, S.cnt[0], S.next, S.offs, false) != 0 ||
             zh_v_build(S.lens + nlit, ndist, S.dist, ZH_V_DIST_BITS, S.sorted_dist, 31u, S.cnt[1], S.next, S.offs, false) != 0) {
            reason = ZH_V_CODELENS;
            break;
         }
         // ---- tokens
         uint32_t lit_val = 0, lit_group = 0;
         bool lit_set = false, lit_any = false;   // lit_set: this lane holds the literal of position lit_group * 64 + lane
         for (;;) {
            zh_v_fill(b);
            if (zh_v_pos(b) > end_bit) {
               reason = ZH_V_STREAM_END;
               break;
            }
            const int sym = zh_v_sym(b, S.lit, ZH_V_LIT_BITS, S.sorted_lit, 511u, S.cnt[0]);
            if (sym < 0 || sym >= 286) {
               reason = ZH_V_SYMBOL;
               break;
            }
            if (sym == ZH_EOB) break;
            if (p >= size) {
               reason = ZH_V_SIZE;
               break;
            }
            if (sym < 256) {
               if (lit_any && (p >> 6) != lit_group) {
                  // p has left the 64-byte stretch the lanes hold literals of: those against the input, one coalesced load
                  zh_v_cmp_settle(cmp);
                  if (lit_set) {
                     cmp.a = in[(lit_group << 6) + lane];
                     cmp.b = lit_val;
                     cmp.pos = (lit_group << 6) + lane;
                     cmp.kind = ZH_V_LITERAL;
                  }
                  lit_set = false;
               }
               lit_group = p >> 6;
               lit_any = true;
               if (lane == (p & 63u)) {
                  lit_val = (uint32_t)sym;
                  lit_set = true;
               }
               p++;
               continue;
            }
            const int li = sym - 257;
            const uint32_t len = zh_lenidx_base(li) + zh_v_take(b, (uint32_t)zh_lenidx_xbits(li));
            zh_v_fill(b);
            const int ds = zh_v_sym(b, S.dist, ZH_V_DIST_BITS, S.sorted_dist, 31u, S.cnt[1]);
            if (ds < 0 || ds >= 30) {
               reason = ZH_V_DISTANCE;
               break;
            }
            const uint32_t dist = zh_dist_base(ds) + zh_v_take(b, (uint32_t)zh_dist_xbits(ds));
            if (dist > ZH_MAX_DIST || dist > back + p) {
               reason = ZH_V_DISTANCE;
               break;
            }
            if (len > size - p) {
               reason = ZH_V_SIZE;
               break;
            }
            for (uint32_t l = lane; l < len; l += 64u) {   // (len <= 258: five rounds at most; the lanes of a round wait for the round before)
               zh_v_cmp_settle(cmp);
               cmp.a = in[p + l];
               cmp.b = in[(int64_t)(p + l) - (int64_t)dist];
               cmp.pos = p + l;
               cmp.kind = ZH_V_MATCH;
            }
            p += len;
         }
         if (reason != ZH_V_OK) break;
         if (lit_any) {
            zh_v_cmp_settle(cmp);
            if (lit_set) {
               cmp.a = in[(lit_group << 6) + lane];
               cmp.b = lit_val;
               cmp.pos = (lit_group << 6) + lane;
               cmp.kind = ZH_V_LITERAL;
            }
         }
      }
      if (reason != ZH_V_OK) break;
      // ---- the block is decoded: now what the compares found
      zh_v_cmp_settle(cmp);
      if (zh_ballot(cmp.bad_at != 0xFFFFFFFFu) != 0) {
         const uint32_t at = zh_wave_min(cmp.bad_at);
         const int who = zh_ctz64(zh_ballot(cmp.bad_at == at));
         reason = zh_readlane(cmp.bad_kind, who & 63);
         *err_pos = at;
         *err_bit = zh_v_pos(b);
         return reason;
      }
      if (zh_v_pos(b) > end_bit) {
         reason = ZH_V_STREAM_END;
         break;
      }
      if (bfinal != ((it.is_final && p == size) ? 1u : 0u)) {
         reason = ZH_V_BFINAL;
         break;
      }
      if (p == size) break;
      if (p == p0 && ++nempty > max_empty) reason = ZH_V_HEADER;
   }
   *err_pos = p;
   *err_bit = zh_v_pos(b);
   return reason;
}

// One wave per sub-block of the last stitched batch, striding: the grid needs no count. files != 0: the batch was stitched as one stream per
// max-block (zh_stitch_scan): a max-block's last sub-block ends within the last byte before the next file's first.
#define ZH_VERIFY_THREADS 64
#ifdef ZH_EMU
#define ZH_VERIFY_WAVES_PER_SIMD
#else
#define ZH_VERIFY_WAVES_PER_SIMD __attribute__((amdgpu_waves_per_eu(3)))   // at most 168 VGPRs: a CU then holds twelve sub-blocks, the chip 3072 (the chains are serial: residency is the throughput)
#endif
__global__ void __launch_bounds__(ZH_VERIFY_THREADS) ZH_VERIFY_WAVES_PER_SIMD
zh_verify_subblocks(const uint32_t *__restrict__ stream, uint64_t stream_cap, const zh_stitch_item_t *__restrict__ items, const zh_subblock_t *__restrict__ subs,
                    const zh_block_t *__restrict__ blocks, uint32_t nblocks, const uint8_t *__restrict__ data, const zh_scan_out_t *__restrict__ scan, const uint64_t *__restrict__ file_off,
                    int files, zh_verify_item_t *out, zh_verify_report_t *report) {
   __shared__ zh_v_lds_t S;
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
               const bool ends = (files && last_of_block) ? ((err_bit + 7u) >> 3) == file_off[sb.block + 1u] : err_bit == (k + 1u < nsubs ? items[k + 1u].dst_bit : end_bit);
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
