// zh_copy.h — the 16-byte mover under zh_zip_copy (zh_zip.h: streams into a ZIP archive's local part) and zh_uz_copy (zh_unzip.h: stored entries out of one).
//
// Source and destination are at byte addresses independent of each other. The destination is whole 16-byte chunks, one store each; a chunk's bytes are put
// together from ALIGNED 16-byte loads — the sixteen bytes that hold its first source byte and, where the source is not aligned like the destination, the sixteen
// behind them — with a byte shift. The caller copies what lies in front of and behind the chunks byte by byte, and answers for the loads: they reach up to 15
// bytes in front of the first source byte and up to 15 behind the last.
#pragma once
#include <zh_platform.h>
#include <stdint.h>

#define ZH_ZIP_SLICE_CHUNKS 512u   // 8 KiB: eight stores a lane
#define ZH_ZIP_UNROLL 2u

#if defined(__HIPCC__) || defined(ZH_EMU)
__device__ __forceinline__ uint32_t zh_zip_shift(uint32_t lo, uint32_t hi, uint32_t sh) { return sh ? (lo >> sh) | (hi << (32u - sh)) : lo; }   // (sh = 0: no shift by 32)

// nchunks chunks to `out` (16-byte aligned) from `s` (any address): of the slices of ZH_ZIP_SLICE_CHUNKS chunks the wave of `lane` takes y, y + yslices, ...
__device__ __forceinline__ void zh_copy_chunks(uint8_t *out, const uint8_t *s, uint32_t nchunks, uint32_t y, uint32_t yslices, uint32_t lane) {
   const uintptr_t mask = ~(uintptr_t)15;
   const uint32_t bs = (uint32_t)((uintptr_t)s & 15u), sh = (bs & 3u) * 8u;
   for (uint32_t sl = y; (uint64_t)sl * ZH_ZIP_SLICE_CHUNKS < nchunks; sl += yslices) {
      const uint32_t end = min(nchunks, (sl + 1) * ZH_ZIP_SLICE_CHUNKS);
      for (uint32_t k0 = sl * ZH_ZIP_SLICE_CHUNKS + lane; k0 < end; k0 += 64 * ZH_ZIP_UNROLL) {
         // ZH_ZIP_UNROLL chunks a lane and round, all their loads in flight before the first store
         uint4 A[ZH_ZIP_UNROLL], B[ZH_ZIP_UNROLL];
#pragma unroll
         for (uint32_t u = 0; u < ZH_ZIP_UNROLL; u++) {
            const uint4 *p = (const uint4 *)((uintptr_t)(s + (uint64_t)16 * (k0 + 64 * u)) & mask);
            A[u] = B[u] = make_uint4(0, 0, 0, 0);
            if (k0 + 64 * u < end) {
               A[u] = p[0];
               if (bs) B[u] = p[1];
            }
         }
#pragma unroll
         for (uint32_t u = 0; u < ZH_ZIP_UNROLL; u++) {
            const uint4 a = A[u], b = B[u];
            uint4 r = a;
            if (bs) {
               uint32_t v0, v1, v2, v3, v4;
               switch (bs >> 2) {
               case 0: v0 = a.x, v1 = a.y, v2 = a.z, v3 = a.w, v4 = b.x; break;
               case 1: v0 = a.y, v1 = a.z, v2 = a.w, v3 = b.x, v4 = b.y; break;
               case 2: v0 = a.z, v1 = a.w, v2 = b.x, v3 = b.y, v4 = b.z; break;
               default: v0 = a.w, v1 = b.x, v2 = b.y, v3 = b.z, v4 = b.w; break;
               }
               r = make_uint4(zh_zip_shift(v0, v1, sh), zh_zip_shift(v1, v2, sh), zh_zip_shift(v2, v3, sh), zh_zip_shift(v3, v4, sh));
            }
            if (k0 + 64 * u < end) *(uint4 *)(out + (uint64_t)16 * (k0 + 64 * u)) = r;
         }
      }
   }
}
#endif
