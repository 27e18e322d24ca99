// zh_frame.h — framed members on the device: the header and trailer bytes around every stream of a files-form assembly (zh_stitch.h).
//
// zh_stitch_scan, given a head and a tail size, leaves that much room in front of and behind every max-block's deflate stream; zh_stitch moves the
// bits; zh_frame_members, behind it on the same stream, fills the room: the gzip / zlib header and trailer exactly as zultra_frame_encode_header /
// zultra_frame_encode_footer write them (frame.c:390-433, 455-480), or a BGZF header (the gzip header with FEXTRA and the 'BC' subfield that holds the
// member's size - 1) and, behind the last member, BGZF's empty end marker. The checksums are finalised here from what zh_crc32_blocks / zh_crc32_small
// left per max-block: the CRC-32's linear part needs the term 0xFFFFFFFF * x^(8n) mod P, the Adler sums need the 1 and the n.
//
// Who writes which byte: a header's last bytes and a trailer's first share dwords with the stream between them, which zh_stitch ORs
// into. The clearing (zh_frame_clear) covers the gaps, zh_stitch touches no gap byte (its plain stores are interior dwords of a sub-block, everything at an edge
// is an OR into zeros), and this kernel runs behind it in stream order and writes single BYTES of the gaps: no byte has two writers, nothing is read back.
#pragma once
#include "zh_stitch.h"

#define ZH_FRAME_RAW 0u
#define ZH_FRAME_ZLIB 1u    // ZULTRA_FLAG_ZLIB_FRAMING
#define ZH_FRAME_GZIP 2u    // ZULTRA_FLAG_GZIP_FRAMING
#define ZH_FRAME_BGZF 4u    // ZULTRA_HIP_FRAME_BGZF
#define ZH_BGZF_MEMBER_MAX 65536u   // BSIZE is a u16 holding size - 1; ISIZE of a BGZF member is at most 65536 as well
#define ZH_BGZF_EOF_SIZE 28u
#define ZH_FRAME_ROOM 32u   // bytes of the stream buffer per max-block for a header and a trailer (BGZF: 18 + 8)

struct zh_member_t {   // = zultra_hip_member_t
   uint64_t off, size;
   uint32_t check, flags;
};

ZH_HD uint32_t zh_frame_head(uint32_t framing) { return framing == ZH_FRAME_GZIP ? 10u : framing == ZH_FRAME_ZLIB ? 2u : framing == ZH_FRAME_BGZF ? 18u : 0u; }
ZH_HD uint32_t zh_frame_tail(uint32_t framing) { return framing == ZH_FRAME_ZLIB ? 4u : framing == ZH_FRAME_RAW ? 0u : 8u; }

// The largest BGZF member a context of max-blocks of max_block_size bytes can produce: zh_stitch_step fails a max-block (the reference's
// ZULTRA_ERROR_DST) as soon as the WHOLE bytes of its stream exceed zh_stitch_blockbuf_cap(max_block_size); up to seven pending bits may follow, which the pad to
// a byte turns into one byte more. So a stream has at most cap + 1 bytes, a member 18 + cap + 1 + 8: at most 65536 for every max_block_size up to 65503.
ZH_HD constexpr uint64_t zh_bgzf_member_bound(uint32_t max_block_size) { return 18 + (1 + (uint64_t)max_block_size + 5 * ((uint64_t)max_block_size / 65535 + 1)) + 1 + 8; }

#if defined(__HIPCC__) || defined(ZH_EMU)
#include <zh_platform.h>

#define ZH_CRC_POLY 0xEDB88320u
// a * b mod P over GF(2), reflected: bit 31 is x^0
__device__ __forceinline__ uint32_t zh_gf2_mulmod(uint32_t a, uint32_t b) {
   uint32_t p = 0;
   for (uint32_t k = 0; k < 32; k++) {
      if (a & (0x80000000u >> k)) p ^= b;
      b = (b >> 1) ^ ((b & 1u) ? ZH_CRC_POLY : 0u);
   }
   return p;
}
// CRC-32 of n bytes from their linear part (zero initial state, no final inversion): the initial 0xFFFFFFFF runs through n zero bytes, which is a
// multiplication by x^(8n) — square-and-multiply over the bits of n —, and the result is inverted (what zultra_crc32_append(0, lin, n) gives on the host)
__device__ __forceinline__ uint32_t zh_crc32_finish(uint32_t lin, uint32_t n) {
   uint32_t q = 0x80000000u >> 8, p = 0x80000000u;   // x^8, x^0
   for (uint32_t m = n; m; m >>= 1) {
      if (m & 1u) p = zh_gf2_mulmod(q, p);
      q = zh_gf2_mulmod(q, q);
   }
   return ~(zh_gf2_mulmod(p, 0xFFFFFFFFu) ^ lin);
}
__device__ __forceinline__ uint32_t zh_adler32_finish(uint32_t sum, uint32_t weighted, uint32_t n) {
   const uint32_t a = (1u + sum) % ZH_ADLER_MOD, b = (n % ZH_ADLER_MOD + weighted) % ZH_ADLER_MOD;
   return (b << 16) | a;
}

__device__ __forceinline__ void zh_put_le(uint8_t *p, uint32_t v, uint32_t nbytes) {
   for (uint32_t k = 0; k < nbytes; k++) p[k] = (uint8_t)(v >> (8 * k));
}

// What a framed assembly clears of the stream buffer, between the scan and the mover: exactly the bytes the members and the end marker will take, rounded up
// to 16 (the buffer has 16 bytes behind stream_cap) — and nothing at all where nothing will be written, so a refused call leaves the buffer as it found it.
#define ZH_FRAME_CLEAR_THREADS 256
__global__ void __launch_bounds__(ZH_FRAME_CLEAR_THREADS)
zh_frame_clear(const zh_scan_out_t *__restrict__ scan, uint64_t stream_cap, uint32_t eof, uint4 *out) {
   if (scan->failed || scan->oversize || ((scan->end_bit + 7) >> 3) + 8 > stream_cap) return;   // (zh_stitch's conditions)
   const uint64_t n16 = (((scan->end_bit + 7) >> 3) + eof + 15) >> 4;
   for (uint64_t k = (uint64_t)blockIdx.x * ZH_FRAME_CLEAR_THREADS + threadIdx.x; k < n16; k += (uint64_t)gridDim.x * ZH_FRAME_CLEAR_THREADS) out[k] = make_uint4(0, 0, 0, 0);
}

// One lane per member, striding; lane nblocks writes the end marker. Writes the stream buffer only where zh_stitch did (the same three conditions), the
// members' records always: with scan->oversize they carry the flags and the host reports -3. Workgroups of up to ZH_FRAME_THREADS lanes (the host may launch fewer).
#define ZH_FRAME_THREADS 64
__global__ void __launch_bounds__(ZH_FRAME_THREADS)
zh_frame_members(const zh_block_t *__restrict__ blocks, uint32_t nblocks, const uint64_t *__restrict__ file_off, const uint32_t *__restrict__ crc, const uint32_t *__restrict__ adler,
                 const zh_scan_out_t *__restrict__ scan, uint64_t stream_cap, uint32_t framing, uint32_t member_max, uint32_t eof, uint8_t *out, zh_member_t *members) {
   if (scan->failed) return;
   const bool write = !scan->oversize && ((scan->end_bit + 7) >> 3) + 8 <= stream_cap;   // (stream_cap: what is left of the buffer in front of the end marker)
   const uint32_t head = zh_frame_head(framing), tail = zh_frame_tail(framing);
   for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b <= nblocks; b += gridDim.x * blockDim.x) {
      if (b == nblocks) {
         if (write && eof) {
            uint8_t *p = out + (file_off[nblocks] - head);
            const uint8_t marker[ZH_BGZF_EOF_SIZE] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (uint32_t k = 0; k < ZH_BGZF_EOF_SIZE; k++) p[k] = marker[k];
         }
         break;
      }
      const uint32_t n = blocks[b].n;
      zh_member_t m;
      m.off = file_off[b] - head;
      m.size = file_off[b + 1] - file_off[b];
      m.check = framing == ZH_FRAME_RAW ? 0u : framing == ZH_FRAME_ZLIB ? zh_adler32_finish(adler[2 * b], adler[2 * b + 1], n) : zh_crc32_finish(crc[b], n);
      m.flags = (member_max && (n > member_max || m.size > member_max)) ? 1u : 0u;
      members[b] = m;
      if (!write || framing == ZH_FRAME_RAW) continue;
      uint8_t *h = out + m.off, *t = out + m.off + m.size - tail;
      if (framing == ZH_FRAME_ZLIB) {
         h[0] = 0x78;   // CMF; FLG: level 3, no dictionary, FCHECK (frame.c:412-433)
         h[1] = 0xda;
         for (uint32_t k = 0; k < 4; k++) t[k] = (uint8_t)(m.check >> (8 * (3 - k)));   // big-endian
      }
      else {
         const bool bgzf = framing == ZH_FRAME_BGZF;
         h[0] = 0x1f;
         h[1] = 0x8b;
         h[2] = 8;
         h[3] = bgzf ? 4 : 0;             // FLG: FEXTRA
         zh_put_le(h + 4, 0, 4);          // MTIME
         h[8] = bgzf ? 0 : 2;             // XFL (frame.c:390-401: 2)
         h[9] = 0xff;                     // OS
         if (bgzf) {
            zh_put_le(h + 10, 6, 2);      // XLEN
            h[12] = 'B';
            h[13] = 'C';
            zh_put_le(h + 14, 2, 2);      // SLEN
            zh_put_le(h + 16, (uint32_t)(m.size - 1), 2);   // BSIZE
         }
         zh_put_le(t, m.check, 4);
         zh_put_le(t + 4, n, 4);          // ISIZE
      }
   }
}
#endif
