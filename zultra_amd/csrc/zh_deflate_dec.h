// zh_deflate_dec.h — the deflate decoder (RFC 1951) under the verify kernel (zh_verify.h) and the inflate kernels (zh_inflate_out.h): everything that
// knows the format and does not know what becomes of the decoded bytes. One wave64 decodes one stream; the decode state (bit position, output
// position) is wave-uniform. What it accepts is what zlib's inflate accepts: over-subscribed and incomplete code sets are rejected, except the
// incomplete set of a single one-bit code; HLIT > 286 and HDIST > 30, a missing end-of-block code, symbols 286 / 287 and 30 / 31, LEN != ~NLEN
// and BTYPE 3 are rejected.
//
//   bit reader   a window of 64 dwords held one per lane (loaded coalesced, read with zh_readlane at a uniform index) feeds a 64-bit hold, 32 bits at
//                a time. Where the dwords come from is the SOURCE, a compile-time parameter: zh_d_stream_src_t is a whole buffer of dwords
//                (verify), zh_d_item_src_t a byte range inside a caller's buffer at any byte address (inflate);
//   tables       per deflate block the wave builds in LDS (zh_d_lds_t, ~3.4 KB) a 9-bit primary table for literals / lengths, 8-bit for distances,
//                7-bit for the code length code, and behind them a canonical length-count walk for the longer codes (zh_d_build, zh_d_sym);
//   zh_d_blocks  the block loop: header bits, BTYPE dispatch, stored header (zh_d_stored_header), table setup (zh_d_tables: the fixed lengths or
//                zh_d_dynamic_lens), token step (zh_d_token). What happens to a literal, a match and a stored run, how much room is left and which
//                reason says that it ran out, how far back a match may reach and what is looked at behind a block is the SINK, the second
//                compile-time parameter; the two sinks (zh_v_sink_t, zh_i_sink_t) are the only decoder code of the two kernels' own.
//
// Prefixes say where a name lives: zh_d_ / ZH_D_ this file, zh_v_ zh_verify.h, zh_i_ zh_inflate_out.h. The reasons keep the names of the public
// list they mirror (ZH_V_*: ZULTRA_HIP_VERIFY_*, which the inflate results use too, and ZH_I_DST_FULL behind it).
//
// The order of the verdicts is the one property in which the two decoders differ, and both orders are behaviour (a report's reason and stream bit):
// it is SRC::end_first, read by zh_d_end_before / zh_d_end_after and at three more places, each marked "order".
//   end_first (inflate)   the end of the data is looked at after every read, and before every other verdict: a cut-off stream is
//                         ZH_V_STREAM_END whatever the zero bits behind its end would decode to (bits that are no code at all: as soon as the
//                         15 bits a code may have reach past the end);
//   !end_first (verify)   the end is looked at once per token, before the token's bits are decoded, and behind the block.
//
// The decoder is total: any byte string gives a verdict and nothing else. Every bit read is bounded by the source's end (dwords behind it read as
// zero, and the position is checked once per token at least), every table index — loads and the stores into S.lens alike — is masked, every loop
// advances the bit position or the output position, both bounded (runs of empty blocks: the sink's block_end). The sinks check every input index,
// every store and every match source before the access.
#pragma once
#include <stdint.h>

#include "zh_common.h"

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

#if defined(__HIPCC__) || defined(ZH_EMU)
#include <zh_platform.h>

#define ZH_D_LIT_BITS 9u
#define ZH_D_DIST_BITS 8u
#define ZH_D_CL_BITS 7u
#define ZH_D_ENTRY(sym, len) ((uint16_t)((sym) | ((len) << 9)))   // symbol < 512, code length 1..15; 0 = no code of at most `bits` bits starts like this

struct zh_d_lds_t {
   uint16_t lit[1u << ZH_D_LIT_BITS];
   uint16_t dist[1u << ZH_D_DIST_BITS];
   uint16_t cl[1u << ZH_D_CL_BITS];
   uint16_t sorted_lit[512];   // symbols in (code length, symbol) order: the canonical walk's answer; 288 used, indexed & 511
   uint16_t sorted_dist[32];   // ... 32 used, indexed & 31 (also the code length code's while the lengths are read)
   uint32_t cnt[2][16];        // codes per length: [0] literals / lengths, [1] distances (and the code length code)
   uint32_t next[16], offs[16];   // builder: first code and first sorted slot of every length
   uint8_t lens[320];
};

static __device__ const uint8_t zh_d_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};   // RFC 1951 3.2.7

// ---- the two sources: dword i of the bit reader's base, zero behind the end of the data ---------------------------------------------------------
struct zh_d_stream_src_t {   // the stream buffer, whole dwords
   static constexpr bool end_first = false;
   const uint32_t *base;
   uint64_t ndw;   // dwords that hold bits of the stream
   __device__ __forceinline__ uint32_t dword(uint64_t i) const { return i < ndw ? base[i] : 0u; }
};
// One item of a caller's byte buffer. The base is the buffer's address aligned down to a dword; the offsets are bytes from it. No byte outside the
// buffer is loaded (its two edge dwords are put together from bytes), and bytes behind the ITEM's own end read as zero.
struct zh_d_item_src_t {
   static constexpr bool end_first = true;
   const uint32_t *base;
   uint64_t buf_lo, buf_hi;   // the caller's whole source buffer
   uint64_t it_hi;            // end of the item
   __device__ __forceinline__ uint32_t dword(uint64_t i) const {
      const uint64_t lo = i * 4u;
      uint32_t w = 0;
      if (lo < it_hi) {
         if (lo >= buf_lo && lo + 4u <= buf_hi)
            w = base[lo >> 2];
         else {   // (the buffer starts or ends inside this dword)
            const uint8_t *s8 = (const uint8_t *)base;
            for (uint32_t k = 0; k < 4u; k++)
               if (lo + k >= buf_lo && lo + k < buf_hi) w |= (uint32_t)s8[lo + k] << (8u * k);
         }
         if (lo + 4u > it_hi) w &= (1u << (8u * (uint32_t)(it_hi - lo))) - 1u;   // (1..3 bytes of the item in it)
      }
      return w;
   }
};

// ---- the bit reader: wave-uniform state, 64 dwords of the source one per lane -------------------------------------------------------------------
struct zh_d_bits_t {
   uint64_t next_dw;   // the dword `hold` is refilled from next (the window covers next_dw - widx .. + 64)
   uint64_t hold;      // the next `have` bits, LSB first
   uint32_t have, widx;
   uint32_t w;         // per lane: dword (window start + lane)
};
template <class SRC>
__device__ __forceinline__ void zh_d_window(zh_d_bits_t &b, const SRC &s) {
   b.w = s.dword(b.next_dw + zh_lane());
   b.widx = 0;
}
// at least 32 bits in hold afterwards (a literal / length code with its extra bits takes 20 at most, a distance 28)
template <class SRC>
__device__ __forceinline__ void zh_d_fill(zh_d_bits_t &b, const SRC &s) {
   if (b.have <= 32u) {
      if (b.widx >= 64u) zh_d_window(b, s);
      b.hold |= (uint64_t)zh_readlane(b.w, (int)(b.widx & 63u)) << b.have;
      b.have += 32u;
      b.widx++;
      b.next_dw++;
   }
}
__device__ __forceinline__ uint64_t zh_d_pos(const zh_d_bits_t &b) { return (b.next_dw << 5) - b.have; }
template <class SRC>
__device__ __forceinline__ void zh_d_seek(zh_d_bits_t &b, const SRC &s, uint64_t bit) {
   b.next_dw = bit >> 5;
   zh_d_window(b, s);
   b.hold = 0;
   b.have = 0;
   zh_d_fill(b, s);
   const uint32_t r = (uint32_t)bit & 31u;
   b.hold >>= r;
   b.have -= r;
}
// n <= 16 bits that are in hold (the caller has filled)
__device__ __forceinline__ uint32_t zh_d_take(zh_d_bits_t &b, uint32_t n) {
   const uint32_t v = (uint32_t)b.hold & ((1u << n) - 1u);
   b.hold >>= n;
   b.have -= n;
   return v;
}
template <class SRC>
__device__ __forceinline__ uint32_t zh_d_get(zh_d_bits_t &b, const SRC &s, uint32_t n) {
   zh_d_fill(b, s);
   return zh_d_take(b, n);
}
// order: has the decode run past the end of the data? !end_first asks before a token's bits are decoded, end_first behind every read — and where
// the bits were no code at all (nocode), as soon as the 15 bits a code may have reach past the end.
template <class SRC>
__device__ __forceinline__ bool zh_d_end_before(const zh_d_bits_t &b, uint64_t end_bit) {
   return !SRC::end_first && zh_d_pos(b) > end_bit;
}
template <class SRC>
__device__ __forceinline__ bool zh_d_end_after(const zh_d_bits_t &b, uint64_t end_bit, bool nocode) {
   return SRC::end_first && zh_d_pos(b) + (nocode ? 15u : 0u) > end_bit;
}

// ---- decode tables of one alphabet ---------------------------------------------------------------------------------------------------
// lens[0 .. n) (values 0..15) -> primary table of 2^tbits entries, the symbols in canonical order, the counts per length. Wave-uniform result:
// 0 = usable (a set without any code included: every decode then fails), 1 = over-subscribed, 2 = incomplete — which zlib accepts only for a
// single code of one bit, and never for the code length code (is_cl).
__device__ __forceinline__ int zh_d_build(const uint8_t *lens, uint32_t n, uint16_t *table, uint32_t tbits, uint16_t *sorted, uint32_t smask, uint32_t *cnt, uint32_t *next,
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
            for (uint32_t j = r; j < (1u << tbits); j += 1u << L) table[j] = ZH_D_ENTRY(s, L);
         }
         c++;
      }
   }
   zh_sync();
   return 0;
}

// next symbol (hold has 15 bits or more, zero bits behind the source's end), -1 where the bits are no code of the set
__device__ __forceinline__ int zh_d_sym(zh_d_bits_t &b, const uint16_t *table, uint32_t tbits, const uint16_t *sorted, uint32_t smask, const uint32_t *cnt) {
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

// ---- the steps of a block --------------------------------------------------------------------------------------------------------------
// Every step returns a reason (wave-uniform); where it is not ZH_V_OK the bit reader stands where the report's stream bit is.

// The code lengths of a dynamic block (RFC 1951 3.2.7) into S.lens[0 .. nlit + ndist).
template <class SRC>
__device__ __forceinline__ uint32_t zh_d_dynamic_lens(zh_d_lds_t &S, zh_d_bits_t &b, const SRC &s, uint64_t end_bit, uint32_t *pnlit, uint32_t *pndist) {
   const uint32_t lane = zh_lane();
   const uint32_t nlit = zh_d_get(b, s, 5) + 257u;
   const uint32_t ndist = zh_d_get(b, s, 5) + 1u;
   const uint32_t ncl = zh_d_get(b, s, 4) + 4u;
   if (zh_d_end_after<SRC>(b, end_bit, false)) return ZH_V_STREAM_END;
   if (nlit > 286u || ndist > 30u) return ZH_V_HEADER;
   if (lane < 19u) S.lens[lane] = 0;
   zh_sync();
   for (uint32_t i = 0; i < ncl; i++) {
      const uint32_t v = zh_d_get(b, s, 3);
      if (lane == 0) S.lens[zh_d_cl_order[i]] = (uint8_t)v;
   }
   if (zh_d_end_after<SRC>(b, end_bit, false)) return ZH_V_STREAM_END;
   zh_sync();
   if (zh_d_build(S.lens, 19, S.cl, ZH_D_CL_BITS, S.sorted_dist, 31u, S.cnt[1], S.next, S.offs, true) != 0) return ZH_V_CODELENS;
   const uint32_t n = nlit + ndist;   // (both alphabets as one run-length coded sequence: a run may cross from the literals into the distances)
   uint32_t i = 0, prev = 0;
   while (i < n) {
      zh_d_fill(b, s);
      if (zh_d_end_before<SRC>(b, end_bit)) return ZH_V_STREAM_END;
      const int sym = zh_d_sym(b, S.cl, ZH_D_CL_BITS, S.sorted_dist, 31u, S.cnt[1]);
      if (sym < 0) return zh_d_end_after<SRC>(b, end_bit, true) ? ZH_V_STREAM_END : ZH_V_CODELENS;
      const bool bad = sym > 18 || (sym == 16 && i == 0);
      if (!SRC::end_first && bad) return ZH_V_CODELENS;   // order: !end_first says so before the repeat's extra bits are taken, end_first behind them and the look at the end
      uint32_t rep = 1, val = (uint32_t)sym;
      if (sym == 16) {
         val = prev;
         rep = 3u + zh_d_take(b, 2);
      }
      else if (sym == 17) {
         val = 0;
         rep = 3u + zh_d_take(b, 3);
      }
      else if (sym >= 18) {
         val = 0;
         rep = 11u + zh_d_take(b, 7);
      }
      if (zh_d_end_after<SRC>(b, end_bit, false)) return ZH_V_STREAM_END;
      if (bad || i + rep > n) return ZH_V_CODELENS;
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

// The tables of a coded block: the fixed code's lengths (btype 1) or the block's own (btype 2), then both alphabets through the builder.
template <class SRC>
__device__ __forceinline__ uint32_t zh_d_tables(zh_d_lds_t &S, zh_d_bits_t &b, const SRC &s, uint64_t end_bit, uint32_t btype) {
   uint32_t nlit = 288, ndist = 32;
   if (btype == 1u) {
      for (uint32_t i = zh_lane(); i < 320u; i += 64u) S.lens[i] = (uint8_t)(i < 288u ? zh_static_lit_len((int)i) : 5);
      zh_sync();
   }
   else {
      const uint32_t reason = zh_d_dynamic_lens(S, b, s, end_bit, &nlit, &ndist);
      if (reason != ZH_V_OK) return reason;
   }
   if (zh_d_build(S.lens, nlit, S.lit, ZH_D_LIT_BITS, S.sorted_lit, 511u, S.cnt[0], S.next, S.offs, false) != 0 ||
       zh_d_build(S.lens + nlit, ndist, S.dist, ZH_D_DIST_BITS, S.sorted_dist, 31u, S.cnt[1], S.next, S.offs, false) != 0)
      return ZH_V_CODELENS;
   return ZH_V_OK;
}

// A stored block's header: LEN and NLEN on the next byte boundary (the pad bits are ignored, RFC 1951 3.2.4). The LEN bytes are
// ((const uint8_t *)s.base)[*pbyte .. + *plen): inside the data and not more than the sink has room for.
template <class SRC, class SINK>
__device__ __forceinline__ uint32_t zh_d_stored_header(zh_d_bits_t &b, const SRC &s, uint64_t end_bit, const SINK &K, uint64_t *pbyte, uint32_t *plen) {
   const uint64_t byte = (zh_d_pos(b) + 7u) >> 3;
   if ((byte + 4u) * 8u > end_bit) return ZH_V_STREAM_END;
   zh_d_seek(b, s, byte * 8u);
   const uint32_t len = zh_d_get(b, s, 16), nlen = zh_d_get(b, s, 16);
   if (len != (~nlen & 0xffffu)) return ZH_V_STORED_LEN;
   const bool past = (byte + 4u + len) * 8u > end_bit, full = len > K.room();
   if (past || full) return (SRC::end_first ? past : !full) ? ZH_V_STREAM_END : SINK::full;   // order: end_first names the end of the data first, !end_first the room
   *pbyte = byte + 4u;
   *plen = len;
   return ZH_V_OK;
}

// One token. *pdist == 0: *pval is a literal, or ZH_EOB; else a match of *pval bytes at distance *pdist, both in range and within the sink's
// reach and room.
template <class SRC, class SINK>
__device__ __forceinline__ uint32_t zh_d_token(zh_d_lds_t &S, zh_d_bits_t &b, const SRC &s, uint64_t end_bit, const SINK &K, uint32_t *pval, uint32_t *pdist) {
   *pdist = 0;
   zh_d_fill(b, s);
   if (zh_d_end_before<SRC>(b, end_bit)) return ZH_V_STREAM_END;
   const int sym = zh_d_sym(b, S.lit, ZH_D_LIT_BITS, S.sorted_lit, 511u, S.cnt[0]);
   if (zh_d_end_after<SRC>(b, end_bit, sym < 0)) return ZH_V_STREAM_END;
   if (sym < 0 || sym >= 286) return ZH_V_SYMBOL;
   *pval = (uint32_t)sym;
   if (sym == ZH_EOB) return ZH_V_OK;
   if (K.room() == 0 && (sym < 256 || !SRC::end_first)) return SINK::full;   // order: without room !end_first refuses a length before its distance is decoded, end_first behind it
   if (sym < 256) return ZH_V_OK;
   const int li = sym - 257;
   const uint32_t len = zh_lenidx_base(li) + zh_d_take(b, (uint32_t)zh_lenidx_xbits(li));
   zh_d_fill(b, s);
   const int ds = zh_d_sym(b, S.dist, ZH_D_DIST_BITS, S.sorted_dist, 31u, S.cnt[1]);
   if (ds < 0 || ds >= 30) return zh_d_end_after<SRC>(b, end_bit, ds < 0) ? ZH_V_STREAM_END : ZH_V_DISTANCE;
   const uint32_t dist = zh_dist_base(ds) + zh_d_take(b, (uint32_t)zh_dist_xbits(ds));
   if (zh_d_end_after<SRC>(b, end_bit, false)) return ZH_V_STREAM_END;
   if (dist > ZH_MAX_DIST || dist > K.reach()) return ZH_V_DISTANCE;
   if (len > K.room()) return SINK::full;
   *pval = len;
   *pdist = dist;
   return ZH_V_OK;
}

// ---- the block loop ----------------------------------------------------------------------------------------------------------------------
// Blocks from where the bit reader stands until the sink says that the last one is done. What a SINK has:
//   full                       the reason for "no room" (ZH_V_SIZE, ZH_I_DST_FULL)
//   room(), reach()            bytes that may still be decoded; how far back a match may reach from here
//   literal(v)                 one byte (room() > 0)
//   match(len, dist)           3 <= len <= min(258, room()), 1 <= dist <= min(ZH_MAX_DIST, reach())
//   stored(bytes, len)         a stored run, len <= room(), the bytes inside the data
//   block_end(past, bfinal, &last)   behind a block; past: the block's bits reach past the end of the data (ZH_V_STREAM_END, wherever in its own
//                              order the sink says so). Returns a reason, or sets last. It bounds the runs of blocks without a byte.
template <class SRC, class SINK>
__device__ __forceinline__ uint32_t zh_d_blocks(zh_d_lds_t &S, zh_d_bits_t &b, const SRC &s, uint64_t end_bit, SINK &K) {
   for (;;) {
      if (zh_d_pos(b) + 3u > end_bit) return ZH_V_STREAM_END;
      const uint32_t hdr = zh_d_get(b, s, 3);
      const uint32_t bfinal = hdr & 1u, btype = hdr >> 1;
      if (btype == 3u) return ZH_V_HEADER;
      if (btype == 0u) {
         uint64_t byte;
         uint32_t len;
         const uint32_t reason = zh_d_stored_header(b, s, end_bit, K, &byte, &len);
         if (reason != ZH_V_OK) return reason;
         K.stored((const uint8_t *)s.base + byte, len);
         if (len) zh_d_seek(b, s, (byte + len) * 8u);
      }
      else {
         uint32_t reason = zh_d_tables(S, b, s, end_bit, btype);
         if (reason != ZH_V_OK) return reason;
         for (;;) {
            uint32_t val, dist;
            reason = zh_d_token(S, b, s, end_bit, K, &val, &dist);
            if (reason != ZH_V_OK) return reason;
            if (dist)
               K.match(val, dist);
            else if (val == ZH_EOB)
               break;
            else
               K.literal(val);
         }
      }
      bool last = false;
      const uint32_t reason = K.block_end(zh_d_pos(b) > end_bit, bfinal, &last);
      if (reason != ZH_V_OK || last) return reason;
   }
}
#endif
