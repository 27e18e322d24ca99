// zh_inflate_check.h — batched inflate of gzip (RFC 1952) and zlib (RFC 1950) MEMBERS: the two kernels that stand around zh_inflate_out.h's.
//
//   zh_frame_heads    one lane per item: the member's header is parsed where it lies (every load bounded by the item's end) and an INNER item —
//                     the deflate stream behind the header, the same destination range — is written for zh_inflate_streams[_dict]; or reason 14.
//   zh_check_members  per item whose stream decoded: the CRC-32 (gzip) or Adler-32 (zlib) of the bytes the inflate kernel wrote, the trailer behind
//                     the stream read and compared, and the final result merged from the three kernels' findings.
//
// The verdict of an item, in this order: 14 (header); the inflate kernel's own reason 1..13, untouched, out_size as that kernel left it; 12 where
// the trailer does not fit in the item (the member is cut off); 15 (checksum); 16 (gzip ISIZE). `check` is the checksum COMPUTED over the output,
// filled whenever the stream decoded.
//
// The ZIP form (zh_unzip.h) has no trailer: the expected CRC-32 and size come from the central directory's record (zh_zip_dirent_t), a stored entry counts as
// decoded, and the order is 17 / 14 (zh_uz_locals), the inflate kernel's reason, 16 (out_size != size), 15 (CRC-32).
//
// The checksum follows zh_stitch.h's zh_crc32_blocks / zh_crc32_small: 256-byte slices, one per thread, aligned to the END of the item's output
// (only slice 0 is short); the CRC byte table and the "append 256 zero bytes" operator in LDS; for Adler-32 the slice sums folded with the
// `after * s1 + s2` weighting. What differs: lengths are 64-bit; the output starts at any byte address and nothing outside
// dst[dst_off .. dst_off + out_size) is loaded — a slice is read as bytes up to the first 16-byte boundary, as 16-byte loads, and as bytes again —;
// only the checksum of the call's framing is computed; and the slices of a round are padded at the FRONT (empty slices have the CRC state 0, which
// every operator maps to 0), so a round is always 256 slices: lane 0 of every wave folds its 64, thread 0 folds the four waves with a second
// operator, "append 16384 zero bytes" (64 folds and 4 in a row instead of 256).
//
// Two forms in one launch, picked per item by the HOST from dst_cap (out_size is only known on the device): items of at most
// ZH_CK_SMALL_MAX bytes lie several to a workgroup, spg threads each (zh_crc32_small's layout: spg a power of two, a group never leaves its wave);
// larger ones take one workgroup each and loop in rounds of 256 x 256 bytes. idx[] lists the small items, then the large ones; the first
// small_blocks workgroups of the grid stride over the groups of small items, the others over the large items.
#pragma once
#include <stdint.h>

#include "zh_inflate_out.h"

#define ZH_M_BAD_FRAME 14u
#define ZH_M_BAD_CHECK 15u
#define ZH_M_BAD_ISIZE 16u
#define ZH_M_RAW 0u    // framing: ZULTRA_FLAG_ZLIB_FRAMING, ZULTRA_FLAG_GZIP_FRAMING (libzultra.h)
#define ZH_M_ZLIB 1u
#define ZH_M_GZIP 2u
#define ZH_M_ZIP 3u    // an entry of a ZIP archive (zh_unzip.h): no trailer, the expected CRC-32 and size stand in the central directory
#define ZH_M_UNSUPPORTED 17u   // (ZIP only)

#define ZH_CK_THREADS 256
#define ZH_CK_SLICE 256u                             // bytes per thread-slice
#define ZH_CK_SMALL_MAX (64u * ZH_CK_SLICE)          // the largest dst_cap of the several-to-a-workgroup form: one wave of slices
#define ZH_CK_TABLE_WORDS (256u + 1024u + 1024u)     // byte table; operator "append ZH_CK_SLICE zero bytes"; operator "append 64 * ZH_CK_SLICE zero bytes"
#define ZH_CK_ADLER_MOD 65521u
#define ZH_FRAME_THREADS 256

// zultra_hip_member_result_t (include/zultra_hip.h)
typedef struct zh_member_result_s {
   uint32_t reason, blocks;
   uint64_t out_size, src_used;
   uint32_t head_size, check;
} zh_member_result_t;

// zultra_hip_zip_dirent_t (include/zultra_hip.h): one record of a ZIP archive's central directory, as zh_unzip.h's index writes it
typedef struct zh_zip_dirent_s {
   uint64_t central_at, local_off, dst_off;   // the record's position in the source; the local header's in the archive; the sum of `size` in front of the record
   uint32_t comp_size, size, crc32, name_len;
   uint16_t method, flags, extra_len, comment_len;
} zh_zip_dirent_t;

#if defined(__HIPCC__) || defined(ZH_EMU)

// ---- headers ---------------------------------------------------------------------------------------------------------------------------------
// CRC-32 of p[0 .. n), bit by bit: one lane, a header of a few bytes, and only where FHCRC is set
__device__ __forceinline__ uint32_t zh_fh_crc32(const uint8_t *p, uint64_t n) {
   uint32_t c = 0xFFFFFFFFu;
   for (uint64_t i = 0; i < n; i++) {
      c ^= p[i];
      for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
   }
   return ~c;
}

// The header of one member p[0 .. sz) -> its size, or ~0 (reason 14). have_dict: the call has a dictionary, dict_id = the Adler-32 of all of it.
__device__ __forceinline__ uint64_t zh_fh_parse(const uint8_t *p, uint64_t sz, uint32_t framing, uint32_t have_dict, uint32_t dict_id) {
   const uint64_t bad = ~0ull;
   if (framing == ZH_M_GZIP) {
      // RFC 1952 2.3: ID1 ID2 CM FLG MTIME(4) XFL OS, then what FLG announces
      if (sz < 10 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || (p[3] & 0xe0)) return bad;
      const uint32_t flg = p[3];
      uint64_t head = 10;
      if (flg & 4u) {   // FEXTRA: XLEN, then XLEN bytes
         if (sz - head < 2) return bad;
         const uint64_t xlen = (uint64_t)p[head] | ((uint64_t)p[head + 1] << 8);
         head += 2;
         if (sz - head < xlen) return bad;
         head += xlen;
      }
      for (uint32_t bit = 8; bit <= 16; bit <<= 1)   // FNAME, FCOMMENT: zero-terminated
         if (flg & bit) {
            while (head < sz && p[head]) head++;
            if (head >= sz) return bad;
            head++;
         }
      if (flg & 2u) {   // FHCRC: the low 16 bits of the CRC-32 of the header in front of it (zlib's inflate checks it too)
         if (sz - head < 2) return bad;
         if ((zh_fh_crc32(p, head) & 0xFFFFu) != ((uint32_t)p[head] | ((uint32_t)p[head + 1] << 8))) return bad;
         head += 2;
      }
      return head;
   }
   if (framing == ZH_M_ZLIB) {
      // RFC 1950 2.2: CM = 8, CINFO <= 7, (CMF * 256 + FLG) % 31 == 0
      if (sz < 2 || (p[0] & 15) != 8 || (p[0] >> 4) > 7 || (((uint32_t)p[0] << 8) | p[1]) % 31u) return bad;
      if (p[1] & 0x20) {   // FDICT: DICTID = the Adler-32 of the WHOLE dictionary
         if (!have_dict || sz < 6) return bad;
         const uint32_t id = ((uint32_t)p[2] << 24) | ((uint32_t)p[3] << 16) | ((uint32_t)p[4] << 8) | p[5];
         return id == dict_id ? 6 : bad;
      }
      return have_dict ? bad : 2;   // (the dictionary kernel has one history length per launch: an item without FDICT belongs in a call without a dictionary)
   }
   return 0;
}

// dict: the result of the one-item checksum batch over the whole dictionary (its `check`), or of the host's own sum; looked at for zlib with a dictionary only
__global__ void __launch_bounds__(ZH_FRAME_THREADS)
zh_frame_heads(const uint8_t *src, uint64_t src_size, const zh_inflate_item_t *__restrict__ items, uint32_t n, uint32_t framing, uint32_t have_dict, const zh_member_result_t *dict,
               zh_inflate_item_t *__restrict__ inner, zh_member_result_t *__restrict__ results) {
   const uint32_t dict_id = (have_dict && framing == ZH_M_ZLIB) ? dict->check : 0u;
   for (uint64_t k = (uint64_t)blockIdx.x * ZH_FRAME_THREADS + threadIdx.x; k < n; k += (uint64_t)gridDim.x * ZH_FRAME_THREADS) {
      const zh_inflate_item_t it = items[k];
      uint64_t head = ~0ull;
      if (it.src_off <= src_size && it.src_size <= src_size - it.src_off)   // (the host has refused anything else)
         head = zh_fh_parse(src + it.src_off, it.src_size, framing, have_dict, dict_id);
      const bool ok = head <= it.src_size && head < 0xFFFFFFFFull;
      zh_inflate_item_t in = it;
      if (ok) {
         in.src_off += head;
         in.src_size -= head;
      }
      else
         in.src_size = in.dst_cap = 0;   // (nothing of it is decoded and nothing is written: the inflate kernel ends such an item with reason 12)
      inner[k] = in;
      zh_member_result_t r;
      r.reason = ok ? 0u : ZH_M_BAD_FRAME;
      r.blocks = 0;
      r.out_size = r.src_used = 0;
      r.head_size = ok ? (uint32_t)head : 0u;
      r.check = 0;
      results[k] = r;
   }
}

// ---- checksums -------------------------------------------------------------------------------------------------------------------------------
struct zh_ck_lds_t {
   uint32_t T[ZH_CK_TABLE_WORDS];   // (CRC-32 only)
   uint32_t part[ZH_CK_THREADS];
   uint32_t wave[ZH_CK_THREADS / 64];
   uint32_t asum[ZH_CK_THREADS][2];   // Adler-32: per group of the workgroup (the large form: row 0)
   uint32_t total;
};

__device__ __forceinline__ uint32_t zh_ck_shift(const uint32_t *T, uint32_t c) {   // T: one of the two operators
   return T[c & 0xff] ^ T[256 + ((c >> 8) & 0xff)] ^ T[512 + ((c >> 16) & 0xff)] ^ T[768 + (c >> 24)];
}

// One slice q[0 .. len), len <= ZH_CK_SLICE, all of it inside the item's output. ADLER: s1 = the sum of the bytes, s2 = the sum of (len - k) * q[k]
// (< 2^24); else c = the CRC state behind the bytes.
template <bool ADLER>
__device__ __forceinline__ void zh_ck_byte(const uint32_t *T, uint32_t d, uint32_t &c, uint32_t &s1, uint32_t &s2) {
   if (ADLER) {
      s1 += d;
      s2 += s1;
   }
   else
      c = (c >> 8) ^ T[(c ^ d) & 0xff];
}
template <bool ADLER>
__device__ __forceinline__ void zh_ck_slice(const uint32_t *T, const uint8_t *q, uint32_t len, uint32_t &c, uint32_t &s1, uint32_t &s2) {
   uint32_t k = 0;
   const uint32_t lead = min(len, (uint32_t)(-(uintptr_t)q & 15u));
   for (; k < lead; k++) zh_ck_byte<ADLER>(T, q[k], c, s1, s2);
   for (; k + 16u <= len; k += 16u) {   // (q + k is 16-byte aligned, and the sixteen bytes lie inside the slice)
      const uint4 v = *(const uint4 *)(q + k);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (uint32_t j = 0; j < 4; j++) {
         zh_ck_byte<ADLER>(T, w[j] & 0xff, c, s1, s2);
         zh_ck_byte<ADLER>(T, (w[j] >> 8) & 0xff, c, s1, s2);
         zh_ck_byte<ADLER>(T, (w[j] >> 16) & 0xff, c, s1, s2);
         zh_ck_byte<ADLER>(T, w[j] >> 24, c, s1, s2);
      }
   }
   for (; k < len; k++) zh_ck_byte<ADLER>(T, q[k], c, s1, s2);
}

// Slice `sl` of an output of n bytes cut into nslices: c / the two sums of the slice as they enter the folds.
template <bool ADLER>
__device__ __forceinline__ void zh_ck_one(const uint32_t *T, const uint8_t *p, uint64_t n, uint64_t nslices, uint64_t sl, uint32_t &c, uint32_t *asum) {
   const uint32_t first = (uint32_t)(n - (nslices - 1) * ZH_CK_SLICE);   // 1..ZH_CK_SLICE bytes
   const uint64_t beg = sl == 0 ? 0 : first + (sl - 1) * ZH_CK_SLICE;
   const uint32_t len = sl == 0 ? first : ZH_CK_SLICE;
   uint32_t s1 = 0, s2 = 0;
   c = sl == 0 ? 0xFFFFFFFFu : 0u;   // (the CRC's initial state goes in with the first byte; the folds are linear behind it)
   zh_ck_slice<ADLER>(T, p + beg, len, c, s1, s2);
   if (ADLER) {
      // weight of byte k of this slice inside the output = n - (beg + k) = (n - beg - len) + (len - k)
      const uint64_t after = (n - beg - len) % ZH_CK_ADLER_MOD;
      atomicAdd(&asum[0], s1 % ZH_CK_ADLER_MOD);   // (at most 256 addends below 65521 between two reductions: no overflow)
      atomicAdd(&asum[1], (uint32_t)((after * (s1 % ZH_CK_ADLER_MOD) + s2) % ZH_CK_ADLER_MOD));
   }
}

// What one item needs of the three kernels' results before its bytes are summed
struct zh_ck_item_t {
   zh_inflate_item_t it;
   zh_inflate_result_t in;
   uint32_t frame_reason, head;
   uint32_t want;   // (ZIP: the CRC-32 the directory names)
   uint64_t n;   // bytes to sum: 0 unless the stream decoded
};
__device__ __forceinline__ zh_ck_item_t zh_ck_fetch(const zh_inflate_item_t *items, const zh_inflate_result_t *inner, const zh_member_result_t *results, uint32_t k, uint64_t dst_size) {
   zh_ck_item_t m;
   m.it = items[k];
   m.in = inner[k];
   m.frame_reason = results[k].reason;
   m.head = results[k].head_size;
   const bool decoded = m.frame_reason == 0 && m.in.reason == 0 && m.it.dst_off <= dst_size && m.it.dst_cap <= dst_size - m.it.dst_off;
   m.n = decoded ? (m.in.out_size < m.it.dst_cap ? m.in.out_size : m.it.dst_cap) : 0;   // (the inflate kernel never writes more than dst_cap)
   m.want = 0;
   return m;
}
// ... of a ZIP entry: its range and what to expect from the dirent; a stored entry that zh_uz_locals has passed counts as decoded, `size` bytes out of comp_size
// (zh_uz_copy has put them there); the inflate kernel's result is a deflated entry's only
__device__ __forceinline__ zh_ck_item_t zh_ck_fetch_zip(const zh_zip_dirent_t *dirents, const zh_inflate_result_t *inner, const zh_member_result_t *results, uint32_t k, uint64_t dst_size) {
   const zh_zip_dirent_t e = dirents[k];
   zh_ck_item_t m;
   m.it.src_off = 0;
   m.it.src_size = e.comp_size;
   m.it.dst_off = e.dst_off;
   m.it.dst_cap = e.size;
   m.frame_reason = results[k].reason;
   m.head = results[k].head_size;
   m.want = e.crc32;
   if (e.method == 8)
      m.in = inner[k];
   else {
      m.in.reason = 0;
      m.in.blocks = 0;
      m.in.out_size = e.size;
      m.in.src_used = e.comp_size;
   }
   const bool decoded = m.frame_reason == 0 && m.in.reason == 0 && m.it.dst_off <= dst_size && m.it.dst_cap <= dst_size - m.it.dst_off;
   m.n = decoded ? (m.in.out_size < m.it.dst_cap ? m.in.out_size : m.it.dst_cap) : 0;
   return m;
}
template <uint32_t FRAMING>
__device__ __forceinline__ zh_ck_item_t zh_ck_fetch_as(const zh_inflate_item_t *items, const zh_zip_dirent_t *dirents, const zh_inflate_result_t *inner, const zh_member_result_t *results, uint32_t k,
                                                       uint64_t dst_size) {
   return FRAMING == ZH_M_ZIP ? zh_ck_fetch_zip(dirents, inner, results, k, dst_size) : zh_ck_fetch(items, inner, results, k, dst_size);
}

// The final result of item k (one thread). sum: the finished CRC-32 / Adler-32 of its output.
template <uint32_t FRAMING>
__device__ __forceinline__ void zh_ck_finish(const zh_ck_item_t &m, const uint8_t *src, uint32_t sum, zh_member_result_t *out) {
   zh_member_result_t r;
   r.blocks = m.in.blocks;
   r.out_size = m.in.out_size;
   r.src_used = (uint64_t)m.head + m.in.src_used;
   r.head_size = m.head;
   r.check = 0;
   if (FRAMING == ZH_M_ZIP) {   // 17 and 14 (zh_uz_locals); the inflate kernel's reason; 16, the size, before 15, the CRC-32: a short output fails both, and 16 says more
      r.src_used = m.in.src_used;   // (the deflate bytes consumed: the header is no part of comp_size)
      if (m.frame_reason) {
         r.reason = m.frame_reason;
         r.blocks = 0;
         r.out_size = r.src_used = 0;
         r.head_size = 0;
      }
      else if (m.in.reason)
         r.reason = m.in.reason;
      else {
         r.check = sum;
         r.reason = r.out_size != m.it.dst_cap ? ZH_M_BAD_ISIZE : sum != m.want ? ZH_M_BAD_CHECK : 0u;
      }
   }
   else if (m.frame_reason) {
      r.reason = m.frame_reason;
      r.blocks = 0;
      r.out_size = r.src_used = 0;
      r.head_size = 0;
   }
   else if (m.in.reason || FRAMING == ZH_M_RAW)
      r.reason = m.in.reason;
   else {
      r.check = sum;
      const uint64_t foot = FRAMING == ZH_M_GZIP ? 8 : 4;
      if (r.src_used > m.it.src_size || m.it.src_size - r.src_used < foot)
         r.reason = ZH_V_STREAM_END;   // the trailer does not fit in the item: the member is cut off
      else {
         const uint8_t *f = src + m.it.src_off + r.src_used;
         r.src_used += foot;
         if (FRAMING == ZH_M_GZIP) {
            const uint32_t crc = f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) | ((uint32_t)f[3] << 24);
            const uint32_t isize = f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16) | ((uint32_t)f[7] << 24);
            r.reason = crc != sum ? ZH_M_BAD_CHECK : isize != (uint32_t)r.out_size ? ZH_M_BAD_ISIZE : 0u;
         }
         else
            r.reason = ((((uint32_t)f[0] << 24) | ((uint32_t)f[1] << 16) | ((uint32_t)f[2] << 8) | f[3]) != sum) ? ZH_M_BAD_CHECK : 0u;
      }
   }
   *out = r;
}

__device__ __forceinline__ uint32_t zh_ck_adler(const uint32_t *asum, uint64_t n) {   // from the two folded sums, the initial (1, 0) put in
   const uint32_t a = (1u + asum[0] % ZH_CK_ADLER_MOD) % ZH_CK_ADLER_MOD;
   const uint32_t b = (uint32_t)((n % ZH_CK_ADLER_MOD + asum[1] % ZH_CK_ADLER_MOD) % ZH_CK_ADLER_MOD);
   return (b << 16) | a;
}

// src / dst: the call's buffers (dst is only read). idx[0 .. nsmall): the items of the several-to-a-workgroup form, spg threads each;
// idx[nsmall .. nsmall + nlarge): the others. tables: ZH_CK_TABLE_WORDS words (gzip and ZIP; else not looked at). dirents: ZIP only, in the place of items.
template <uint32_t FRAMING>
__global__ void __launch_bounds__(ZH_CK_THREADS)
zh_check_members(const uint8_t *src, const uint8_t *dst, uint64_t dst_size, const zh_inflate_item_t *__restrict__ items, const zh_inflate_result_t *__restrict__ inner,
                 zh_member_result_t *results, const uint32_t *__restrict__ idx, uint32_t nsmall, uint32_t nlarge, uint32_t spg, uint32_t small_blocks, const uint32_t *__restrict__ tables,
                 const zh_zip_dirent_t *__restrict__ dirents) {
   constexpr bool ADLER = FRAMING == ZH_M_ZLIB;
   const uint32_t tid = threadIdx.x;
   if (FRAMING == ZH_M_RAW) {   // nothing to sum: one thread per item puts the result together
      const uint32_t n = nsmall + nlarge;
      for (uint64_t k = (uint64_t)blockIdx.x * ZH_CK_THREADS + tid; k < n; k += (uint64_t)gridDim.x * ZH_CK_THREADS)
         zh_ck_finish<FRAMING>(zh_ck_fetch(items, inner, results, (uint32_t)k, dst_size), src, 0u, results + k);   // (raw has no ZIP form)
      return;
   }
   __shared__ zh_ck_lds_t S;
   if (FRAMING == ZH_M_GZIP || FRAMING == ZH_M_ZIP) {
      for (uint32_t k = tid; k < ZH_CK_TABLE_WORDS; k += ZH_CK_THREADS) S.T[k] = tables[k];
   }
   if (blockIdx.x < small_blocks) {
      // ---- several items to the workgroup: thread t works on item g = t / spg of its group of `per`, slot t % spg
      const uint32_t per = ZH_CK_THREADS / spg, g = tid / spg, slot = tid % spg;
      const uint32_t ngroups = (nsmall + per - 1) / per;
      for (uint32_t grp = blockIdx.x; grp < ngroups; grp += small_blocks) {
         if (tid < per) S.asum[tid][0] = S.asum[tid][1] = 0;
         __syncthreads();
         const uint32_t at = grp * per + g;
         const bool live = at < nsmall;
         zh_ck_item_t m;
         m.n = 0;
         uint32_t k = 0, c = 0;
         uint64_t nslices = 0;
         if (live) {
            k = idx[at];
            m = zh_ck_fetch_as<FRAMING>(items, dirents, inner, results, k, dst_size);
            nslices = (m.n + ZH_CK_SLICE - 1) / ZH_CK_SLICE;
            if (nslices > spg) m.n = nslices = 0;   // (dst_cap <= spg * ZH_CK_SLICE, as the host chose spg: never)
            const uint32_t pad = spg - (uint32_t)nslices;   // empty slots in front: their state 0 stays 0 under the operator
            if (slot >= pad) zh_ck_one<ADLER>(S.T, dst + m.it.dst_off, m.n, nslices, slot - pad, c, S.asum[g]);
         }
         S.part[tid] = c;
         __syncthreads();
         if (live && slot == 0) {
            uint32_t sum;
            if (ADLER)
               sum = zh_ck_adler(S.asum[g], m.n);
            else {
               uint32_t total = 0;
               for (uint32_t j = 0; j < spg; j++) total = zh_ck_shift(S.T + 256, total) ^ S.part[g * spg + j];
               sum = m.n ? ~total : 0u;
            }
            zh_ck_finish<FRAMING>(m, src, sum, results + k);
         }
         __syncthreads();   // (part and asum are the next group's)
      }
      return;
   }
   // ---- one item to the workgroup, in rounds of ZH_CK_THREADS slices; the first round is the one padded in front
   const uint32_t large_blocks = gridDim.x - small_blocks;
   for (uint32_t at = blockIdx.x - small_blocks; at < nlarge; at += large_blocks) {
      const uint32_t k = idx[nsmall + at];
      const zh_ck_item_t m = zh_ck_fetch_as<FRAMING>(items, dirents, inner, results, k, dst_size);
      const uint64_t nslices = (m.n + ZH_CK_SLICE - 1) / ZH_CK_SLICE;
      const uint64_t nrounds = (nslices + ZH_CK_THREADS - 1) / ZH_CK_THREADS;
      const uint64_t pad = nrounds * ZH_CK_THREADS - nslices;
      if (tid < 2) S.asum[0][tid] = 0;
      if (tid == 0) S.total = 0;
      __syncthreads();
      for (uint64_t round = 0; round < nrounds; round++) {
         const uint64_t v = round * ZH_CK_THREADS + tid;
         uint32_t c = 0;
         if (v >= pad) zh_ck_one<ADLER>(S.T, dst + m.it.dst_off, m.n, nslices, v - pad, c, S.asum[0]);
         if (ADLER) {
            __syncthreads();
            if (tid < 2) S.asum[0][tid] %= ZH_CK_ADLER_MOD;
            __syncthreads();
         }
         else {
            S.part[tid] = c;
            __syncthreads();
            if ((tid & 63u) == 0) {   // the wave's 64 slices
               uint32_t t = 0;
               for (uint32_t j = 0; j < 64; j++) t = zh_ck_shift(S.T + 256, t) ^ S.part[tid + j];
               S.wave[tid >> 6] = t;
            }
            __syncthreads();
            if (tid == 0) {           // ... and the four waves behind what the rounds before have left
               uint32_t t = S.total;
               for (uint32_t w = 0; w < ZH_CK_THREADS / 64; w++) t = zh_ck_shift(S.T + 256 + 1024, t) ^ S.wave[w];
               S.total = t;
            }
            __syncthreads();
         }
      }
      if (tid == 0) zh_ck_finish<FRAMING>(m, src, ADLER ? zh_ck_adler(S.asum[0], m.n) : (m.n ? ~S.total : 0u), results + k);
      __syncthreads();   // (asum and total are the next item's)
   }
}
#endif
