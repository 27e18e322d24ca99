// tests/emu/inflate_range_main.cpp — TEST INFRASTRUCTURE ONLY: zultra_hip_inflate_range in an executable of its own, built with AddressSanitizer and UBSan
// over the emulator build of the device layer (tests/emu/build_emu.py: _build_program; tests/test_inflate_range_emu.py writes the case file and runs it).
//
//    inflate_range_main <case file>
//
// The case file: u64 S, the S bytes of a BGZF file; u64 F, the F bytes of its output; u64 n, then n pairs u64 first, u64 nbytes. Every range runs under the tile
// sizes 32, 100, 256 and the default, each with and without ZULTRA_HIP_GRID_CAP=8. Source, destination and results are heap blocks of exactly the size the
// call may touch, used in place (device memory is host memory here): the source S bytes, the destination out_size bytes, the results range_members records —
// a first call without room learns the two counts. The bytes must be those of the output; any access outside a block is the sanitizers' to report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/zultra_hip.h"

static uint64_t get64(FILE *f) {
   uint64_t v = 0;
   if (fread(&v, 8, 1, f) != 1) {
      fprintf(stderr, "short case file\n");
      exit(2);
   }
   return v;
}
static std::vector<uint8_t> get_bytes(FILE *f) {
   std::vector<uint8_t> b((size_t)get64(f));
   if (!b.empty() && fread(b.data(), 1, b.size(), f) != b.size()) {
      fprintf(stderr, "short case file\n");
      exit(2);
   }
   return b;
}

int main(int argc, char **argv) {
   FILE *f = argc == 2 ? fopen(argv[1], "rb") : NULL;
   if (!f) {
      fprintf(stderr, "usage: %s <case file>\n", argv[0]);
      return 2;
   }
   const std::vector<uint8_t> file = get_bytes(f), want = get_bytes(f);
   const uint64_t nranges = get64(f);
   std::vector<uint64_t> ranges(2 * (size_t)nranges);
   for (uint64_t &v : ranges) v = get64(f);
   fclose(f);
   static const char *const tiles[] = {"32", "100", "256", NULL};
   uint64_t runs = 0, bad = 0;
   for (int t = 0; t < 4; t++)
      for (int capped = 0; capped < 2; capped++) {
         if (tiles[t]) setenv("ZULTRA_HIP_INDEX_TILE", tiles[t], 1);
         else unsetenv("ZULTRA_HIP_INDEX_TILE");
         if (capped) setenv("ZULTRA_HIP_GRID_CAP", "8", 1);
         else unsetenv("ZULTRA_HIP_GRID_CAP");
         for (uint64_t r = 0; r < nranges; r++) {
            const uint64_t first = ranges[2 * r], nbytes = ranges[2 * r + 1];
            const uint64_t lo = first < want.size() ? first : want.size();
            const uint64_t hi = nbytes > ~0ull - first || first + nbytes > want.size() ? want.size() : first + nbytes;
            uint8_t *src = (uint8_t *)malloc(file.size());
            memcpy(src, file.data(), file.size());
            uint8_t none = 0;
            zultra_hip_range_result_t q, res;
            const int qrc = zultra_hip_inflate_range(0, src, file.size(), 1, first, nbytes, &none, 0, 1, &q, NULL, 0, NULL);   // no room: the counts
            bool ok = q.out_size == hi - lo && (hi == lo ? qrc == 0 && q.range_members == 0 : qrc == -1 && q.stop == 4 && q.range_members > 0);
            uint8_t *dst = (uint8_t *)malloc((size_t)q.out_size ? (size_t)q.out_size : 1);
            zultra_hip_member_result_t *results = (zultra_hip_member_result_t *)malloc(q.range_members ? q.range_members * sizeof(zultra_hip_member_result_t) : 1);
            const int rc = zultra_hip_inflate_range(0, src, file.size(), 1, first, nbytes, dst, (size_t)q.out_size, 1, &res, results, q.range_members, NULL);
            ok = ok && rc == 0 && res.out_size == q.out_size && res.range_members == q.range_members && res.first_member == q.first_member &&
                 (q.out_size == 0 || memcmp(dst, want.data() + lo, (size_t)q.out_size) == 0);
            for (uint32_t k = 0; ok && k < res.range_members; k++) ok = results[k].reason == 0;
            if (!ok) {
               bad++;
               fprintf(stderr, "tile %s cap %d range %llu + %llu: rc %d / %d, out_size %llu, members %u\n", tiles[t] ? tiles[t] : "default", capped, (unsigned long long)first,
                       (unsigned long long)nbytes, qrc, rc, (unsigned long long)res.out_size, res.range_members);
            }
            runs++;
            free(results);
            free(dst);
            free(src);
         }
      }
   printf("%llu runs, %llu failed\n", (unsigned long long)runs, (unsigned long long)bad);
   return bad ? 1 : 0;
}
