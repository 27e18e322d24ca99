// TEST INFRASTRUCTURE: a stand-alone program around zultra_memory_compress, linked with the product's sources in the emulator configuration and built with
// AddressSanitizer and UBSan (build_emu.build_notes_program): out-of-range reads and writes of the kernels' logic — the matchfinder walking a part of the
// 6-gram order that nobody wrote — are reported where they happen. Nothing of it is loaded into Python.
//
//    mf_notes_main FILE BLOCK_SIZE FLAGS MF_CAP   > stream
//
// FLAGS: 0 raw deflate, 1 zlib, 2 gzip (libzultra.h); MF_CAP: ZULTRA_HIP_MF_CAP for the contexts the call creates, 0 = leave the environment alone.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../include/libzultra.h"

int main(int argc, char **argv) {
   if (argc != 5) {
      fprintf(stderr, "usage: %s FILE BLOCK_SIZE FLAGS MF_CAP\n", argv[0]);
      return 2;
   }
   const unsigned block = (unsigned)strtoul(argv[2], NULL, 10), flags = (unsigned)strtoul(argv[3], NULL, 10);
   if (strtoul(argv[4], NULL, 10) != 0) setenv("ZULTRA_HIP_MF_CAP", argv[4], 1);   // (before the first call: read when a context is created)
   FILE *f = fopen(argv[1], "rb");
   if (!f) {
      perror(argv[1]);
      return 2;
   }
   std::vector<unsigned char> in;
   unsigned char buf[65536];
   for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) in.insert(in.end(), buf, buf + got);
   fclose(f);
   std::vector<unsigned char> out(zultra_memory_bound(in.size(), flags, block));
   const size_t n = zultra_memory_compress(in.data(), in.size(), out.data(), out.size(), flags, block);
   if (n == (size_t)-1) {
      fprintf(stderr, "zultra_memory_compress failed\n");
      return 1;
   }
   if (fwrite(out.data(), 1, n, stdout) != n) return 1;
   zultra_release_cached_contexts();
   return 0;
}
