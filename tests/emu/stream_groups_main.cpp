// tests/emu/stream_groups_main.cpp — TEST INFRASTRUCTURE ONLY: the grouped assembly (zultra_hip_frame_streams, zultra_hip_zip_streams) in an executable of its own,
// built with AddressSanitizer and UBSan over the emulator build of the device layer (tests/emu/build_emu.py: _build_program; tests/test_stream_groups_emu.py writes
// the case file and runs it).
//
//    stream_groups_main <case file>
//
// The case file: u64 n and the n bytes of a batch's input; u64 B, then B max-blocks as u64 win_off, prev, n; u64 S, then the S streams' first max-blocks as u64;
// then for the framings 0, 1, 2: u64 size and the bytes the stream buffer must hold, the reference's members back to back. The batch is compressed once. Per
// framing the stream buffer must hold those bytes, the members' offsets and sizes must tile them, and the batch must verify. Then the refusals: with both buffers
// marked, every invalid grouping returns -1 from both calls and leaves every marked byte as it was. Any access outside a block is the sanitizers' to report.
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
   const std::vector<uint8_t> data = get_bytes(f);
   std::vector<zultra_hip_block_t> blocks((size_t)get64(f));
   for (zultra_hip_block_t &b : blocks) {
      b.win_off = get64(f);
      b.prev = (uint32_t)get64(f);
      b.n = (uint32_t)get64(f);
   }
   std::vector<uint32_t> first((size_t)get64(f));
   for (uint32_t &v : first) v = (uint32_t)get64(f);
   std::vector<uint8_t> want[3];
   for (int k = 0; k < 3; k++) want[k] = get_bytes(f);
   fclose(f);

   const uint32_t B = (uint32_t)blocks.size(), S = (uint32_t)first.size();
   unsigned bad = 0;
   zultra_hip_ctx_t *c = zultra_hip_create(0, 32768, B);
   if (!c || zultra_hip_compress_blocks(c, data.data(), data.size(), 0, blocks.data(), B) <= 0) {
      fprintf(stderr, "no batch: %s\n", c ? zultra_hip_last_error(c) : "no context");
      return 1;
   }
   std::vector<zultra_hip_member_t> members(S);
   static const unsigned framings[3] = {0, 1, 2};
   for (int k = 0; k < 3; k++) {
      uint64_t total = 0, at = 0;
      const int rc = zultra_hip_frame_streams(c, first.data(), S, framings[k], members.data(), &total);
      bool ok = rc == 0 && total == want[k].size();
      std::vector<uint8_t> got((size_t)total ? (size_t)total : 1);   // (exactly the bytes the call reports)
      ok = ok && zultra_hip_stream_read(c, got.data(), 0, (size_t)total) == 0 && memcmp(got.data(), want[k].data(), (size_t)total) == 0;
      for (uint32_t s = 0; ok && s < S; s++) {
         ok = members[s].off == at && members[s].flags == 0;
         at += members[s].size;
      }
      zultra_hip_verify_t v;
      ok = ok && at == total && zultra_hip_verify_device(c, &v) == 0 && v.verified_bytes == data.size();
      if (!ok) {
         bad++;
         fprintf(stderr, "framing %u: rc %d, %llu bytes of %llu: %s\n", framings[k], rc, (unsigned long long)total, (unsigned long long)want[k].size(), zultra_hip_last_error(c));
      }
   }

   // the refusals, both buffers marked
   std::vector<uint8_t> names(S + 1, 'n');
   std::vector<uint32_t> name_off(S + 2);
   for (uint32_t s = 0; s <= S + 1; s++) name_off[s] = s;
   uint64_t local = 0, central = 0, central_at = 0;
   if (zultra_hip_zip_streams(c, first.data(), S, names.data(), name_off.data(), NULL, S, 0, 0, NULL, &local, &central) != 0) {
      fprintf(stderr, "zip_streams: %s\n", zultra_hip_last_error(c));
      return 1;
   }
   uint8_t *zip = (uint8_t *)zultra_hip_zip_device(c, &central_at);   // (device memory is host memory here)
   std::vector<uint8_t> mark_s(data.size() + 256), mark_z((size_t)(central_at + central)), now_s(mark_s.size());
   for (size_t i = 0; i < mark_s.size(); i++) mark_s[i] = (uint8_t)(i * 7 + 3);
   for (size_t i = 0; i < mark_z.size(); i++) mark_z[i] = (uint8_t)(i * 11 + 5);
   zultra_hip_stream_write(c, mark_s.data(), 0, mark_s.size());
   memcpy(zip, mark_z.data(), mark_z.size());
   struct refusal_t {
      const char *what;
      std::vector<uint32_t> first;
      unsigned framing;
   };
   std::vector<refusal_t> refusals;
   refusals.push_back({"stream_first[0] != 0", {1, B - 1}, 2});
   refusals.push_back({"a non-increasing index", {0, B - 1, B - 1}, 2});
   refusals.push_back({"an index past the batch", {0, 1, B}, 2});
   {
      std::vector<uint32_t> every(B);   // (the case has a stream of several max-blocks: some block of these has history)
      for (uint32_t b = 0; b < B; b++) every[b] = b;
      refusals.push_back({"a stream's first block with history", every, 2});
   }
   refusals.push_back({"BGZF", first, ZULTRA_HIP_FRAME_BGZF});
   refusals.push_back({"nstreams == 0", {}, 2});
   for (const refusal_t &r : refusals) {
      uint64_t total = 0;
      const uint32_t n = (uint32_t)r.first.size();
      std::vector<zultra_hip_member_t> m(n ? n : 1);
      bool ok = zultra_hip_frame_streams(c, n ? r.first.data() : NULL, n, r.framing, m.data(), &total) == -1;
      if (r.framing != ZULTRA_HIP_FRAME_BGZF)
         ok = ok && zultra_hip_zip_streams(c, n ? r.first.data() : NULL, n, names.data(), name_off.data(), NULL, n && n <= S + 1 ? n : 1, 0, 0, NULL, &local, &central) == -1;
      ok = ok && zultra_hip_stream_read(c, now_s.data(), 0, now_s.size()) == 0 && now_s == mark_s && memcmp(zip, mark_z.data(), mark_z.size()) == 0;
      if (!ok) {
         bad++;
         fprintf(stderr, "not refused, or a refused call has written: %s\n", r.what);
      }
   }
   zultra_hip_destroy(c);
   printf("3 framings, %u refusals, %u failed\n", (unsigned)refusals.size(), bad);
   return bad ? 1 : 0;
}
