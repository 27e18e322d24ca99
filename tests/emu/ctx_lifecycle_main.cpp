// TEST INFRASTRUCTURE: a stand-alone program that creates, uses and destroys device contexts, linked with the product's sources in the emulator configuration and
// built with AddressSanitizer, UBSan and LeakSanitizer (build_emu.build_lifecycle_program). In the emulator every hipMalloc is a malloc: a buffer that
// zultra_hip_destroy's walk of the context's buffer list (zh_device.hip, ZH_CTX_BUFFERS) misses is reported at exit, where it was allocated. Nothing of it is
// loaded into Python.
//
//    ctx_lifecycle_main        (no arguments; exit status 0 and nothing on stderr when all is well)
//
// A context of max-blocks (32768 x 2) and a files context (512 x 3) each run one small batch and then every call that allocates on first use or grows a
// buffer — verify, framed members, the files form, zip members (twice, the second call with longer names), both staging slots (twice, the second larger);
// one context is created and destroyed with ZULTRA_HIP_CHAIN_TRACE=1; and all of it twice.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/zultra_hip.h"

#define CHECK(cond)                                                       \
   do {                                                                   \
      if (!(cond)) {                                                      \
         fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
         return 1;                                                        \
      }                                                                   \
   } while (0)

static int use_and_destroy(zultra_hip_ctx_t *c, bool files) {
   CHECK(c != NULL);
   std::vector<unsigned char> data(600);
   for (size_t i = 0; i < data.size(); i++) data[i] = (unsigned char)("the quick brown fox "[i % 20] + (i / 97) % 3);
   uint64_t file_off[3] = {0, 0, 0};
   if (files) {
      const uint64_t offsets[2] = {0, 300};
      const uint32_t sizes[2] = {300, 300};
      CHECK(zultra_hip_compress_files(c, data.data(), data.size(), 0, offsets, sizes, 2, file_off) == 2);
   }
   else {
      const zultra_hip_block_t blocks[2] = {{0, 0, 300}, {300, 0, 300}};
      CHECK(zultra_hip_compress_blocks(c, data.data(), data.size(), 0, blocks, 2) > 0);
      zultra_hip_bitstate_t state = {0, 0};
      uint64_t end_bit = 0;
      CHECK(zultra_hip_stitch_device(c, &state, 1, &end_bit) == 0 && end_bit > 0);
   }
   zultra_hip_verify_t report;
   CHECK(zultra_hip_verify_device(c, &report) == 0);
   zultra_hip_member_t members[2];
   uint64_t total = 0;
   CHECK(zultra_hip_frame_members(c, 2 /* gzip */, 0, members, &total) == 0 && total > 0);
   CHECK(zultra_hip_stitch_files(c, file_off) == 0 && file_off[2] > file_off[1] && file_off[1] > file_off[0]);
   for (int round = 0; round < 2; round++) {
      const char *names = round ? "a/rather/longer/name/for/the/first.txt+the/second/one.txt" : "a.txtb.txt";
      const uint32_t cut = round ? (uint32_t)(strchr(names, '+') - names) : 5u;
      const uint32_t name_off[3] = {0, cut, (uint32_t)strlen(names)};
      zultra_hip_zip_entry_t entries[2];
      uint64_t local_bytes = 0, central_bytes = 0;
      CHECK(zultra_hip_zip_members(c, names, name_off, NULL, 2, 0, 0, entries, &local_bytes, &central_bytes) == 0 && local_bytes > 0 && central_bytes > 0);
   }
   for (int round = 0; round < 2; round++)
      for (int which = 0; which < 2; which++) {
         void *p = zultra_hip_staging(c, which, (size_t)4096 << round);
         CHECK(p != NULL);
         memset(p, 0, (size_t)4096 << round);
      }
   zultra_hip_destroy(c);
   return 0;
}

int main(void) {
   for (int pass = 0; pass < 2; pass++) {
      unsetenv("ZULTRA_HIP_CHAIN_TRACE");
      if (use_and_destroy(zultra_hip_create(0, 32768, 2), false)) return 1;
      if (use_and_destroy(zultra_hip_create_files(0, 512, 3), true)) return 1;
      setenv("ZULTRA_HIP_CHAIN_TRACE", "1", 1);   // (read when a context is created)
      zultra_hip_ctx_t *traced = zultra_hip_create(0, 32768, 2);
      CHECK(traced != NULL);
      zultra_hip_destroy(traced);
   }
   return 0;
}
