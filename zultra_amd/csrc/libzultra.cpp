// libzultra.cpp — the drop-in libzultra API (include/libzultra.h) on top of the MI355X device layer.
//
// Host C++ mirror of reference src/libzultra.c (stream state machine, :200-514; in-memory entry, :576-619),
// src/frame.c (gzip / zlib / raw framing and checksums) and src/dictionary.c. The per-max-block section of the
// reference's loop (:287-403) is replaced by batched calls into include/zultra_hip.h; what depends on the running
// bit phase (3 header bits, stored fallback, bit carry, :327-398 and :414-436) is zultra_hip_stitch below.
// There is no CPU implementation of the hot path in this library: without a HIP device, stream init fails.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "../../include/libzultra.h"
#include "../../include/zultra_hip.h"
#include "zh_host.h"

// ================================================================================================================
// Framing and checksums (reference src/frame.c)
// ================================================================================================================

static uint32_t g_crc_tab[8][256];
static std::once_flag g_crc_once;

static void crc_init() {
   for (uint32_t i = 0; i < 256; i++) {
      uint32_t c = i;
      for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1) ? 0xEDB88320u : 0);
      g_crc_tab[0][i] = c;
   }
   for (uint32_t i = 0; i < 256; i++)
      for (int t = 1; t < 8; t++) g_crc_tab[t][i] = (g_crc_tab[t - 1][i] >> 8) ^ g_crc_tab[0][g_crc_tab[t - 1][i] & 0xff];
}

// CRC-32 (reflected 0xEDB88320), slicing-by-8; same function of the data as frame.c:324-354.
static uint32_t crc32_update(uint32_t crc, const uint8_t *p, size_t n) {
   std::call_once(g_crc_once, crc_init);
   crc = ~crc;
   while (n && ((uintptr_t)p & 7)) {
      crc = (crc >> 8) ^ g_crc_tab[0][(crc ^ *p++) & 0xff];
      n--;
   }
   while (n >= 8) {
      uint64_t v;
      memcpy(&v, p, 8);
      v ^= crc;
      crc = g_crc_tab[7][v & 0xff] ^ g_crc_tab[6][(v >> 8) & 0xff] ^ g_crc_tab[5][(v >> 16) & 0xff] ^ g_crc_tab[4][(v >> 24) & 0xff] ^
            g_crc_tab[3][(v >> 32) & 0xff] ^ g_crc_tab[2][(v >> 40) & 0xff] ^ g_crc_tab[1][(v >> 48) & 0xff] ^ g_crc_tab[0][v >> 56];
      p += 8;
      n -= 8;
   }
   while (n--) crc = (crc >> 8) ^ g_crc_tab[0][(crc ^ *p++) & 0xff];
   return ~crc;
}

// ---- folding device-computed per-block CRCs into the running gzip checksum -----------------------------------------
// With R(s, D) the raw register after feeding D from state s, R(s, D) = Z_n(s) ^ R(0, D) (n = |D|, Z_n = "feed n zero
// bytes", linear over GF(2)); the device returns R(0, block). Z_n is kept as a 32x32 bit matrix per length.
namespace {
struct CrcShiftOp {
   uint32_t col[32];   // image of each state bit
   uint32_t apply(uint32_t v) const {
      uint32_t r = 0;
      for (int b = 0; v; v >>= 1, b++)
         if (v & 1) r ^= col[b];
      return r;
   }
};
static void op_square(CrcShiftOp &dst, const CrcShiftOp &src) {
   for (int b = 0; b < 32; b++) dst.col[b] = src.apply(src.col[b]);
}
static CrcShiftOp crc_shift_op(size_t nbytes) {
   std::call_once(g_crc_once, crc_init);
   CrcShiftOp pw, res, tmp;
   for (int b = 0; b < 32; b++) {           // one zero byte
      uint32_t v = 1u << b;
      pw.col[b] = (v >> 8) ^ g_crc_tab[0][v & 0xff];
      res.col[b] = 1u << b;                  // identity
   }
   for (size_t n = nbytes; n; n >>= 1) {
      if (n & 1) {
         for (int b = 0; b < 32; b++) tmp.col[b] = pw.apply(res.col[b]);
         res = tmp;
      }
      op_square(tmp, pw);
      pw = tmp;
   }
   return res;
}
static std::mutex g_op_mutex;
static size_t g_op_len[4] = {0, 0, 0, 0};
static CrcShiftOp g_op[4];
static int g_op_next = 0;
}   // namespace

extern "C" uint32_t zultra_crc32_append(uint32_t crc, uint32_t block_linear_crc, size_t block_len) {
   CrcShiftOp op;
   {
      std::lock_guard<std::mutex> lk(g_op_mutex);
      int hit = -1;
      for (int i = 0; i < 4; i++)
         if (g_op_len[i] == block_len && block_len) hit = i;
      if (hit < 0) {
         hit = g_op_next;
         g_op_next = (g_op_next + 1) & 3;
         g_op[hit] = crc_shift_op(block_len);
         g_op_len[hit] = block_len;
      }
      op = g_op[hit];
   }
   return ~(op.apply(~crc) ^ block_linear_crc);
}

extern "C" uint32_t zultra_crc32_append_many(uint32_t crc, const uint32_t *block_linear_crc, const uint32_t *block_len, uint32_t nblocks) {
   for (uint32_t b = 0; b < nblocks; b++) crc = zultra_crc32_append(crc, block_linear_crc[b], block_len[b]);
   return crc;
}

extern "C" uint32_t zultra_adler32_append(uint32_t adler, uint32_t block_sum, uint32_t block_weighted_sum, size_t block_len) {
   const uint64_t M = 65521;
   const uint64_t a = adler & 0xffff, b = (adler >> 16) & 0xffff;
   const uint64_t b2 = (b + (uint64_t)(block_len % M) * a + block_weighted_sum) % M;
   const uint64_t a2 = (a + block_sum) % M;
   return (uint32_t)((b2 << 16) | a2);
}

// Adler-32 (frame.c:74-138): sums modulo 65521, reduced every 5552 bytes.
static uint32_t adler32_update(uint32_t adler, const uint8_t *p, size_t n) {
   uint32_t a = adler & 0xffff, b = (adler >> 16) & 0xffff;
   while (n) {
      size_t chunk = n > 5552 ? 5552 : n;
      for (size_t k = 0; k < chunk; k++) {
         a += p[k];
         b += a;
      }
      a %= 65521u;
      b %= 65521u;
      p += chunk;
      n -= chunk;
   }
   return a | (b << 16);
}

extern "C" int zultra_frame_get_header_size(const unsigned int nFlags, const void *pDict, const int nDictSize) {
   if (nFlags & ZULTRA_FLAG_GZIP_FRAMING) return 10;
   if (nFlags & ZULTRA_FLAG_ZLIB_FRAMING) return (pDict && nDictSize) ? 6 : 2;
   return 0;
}

extern "C" int zultra_frame_encode_header(unsigned char *p, const int nMax, const unsigned int nFlags, const void *pDict,
                                          const int nDictSize) {
   if (nFlags & ZULTRA_FLAG_GZIP_FRAMING) {
      // RFC 1952: magic, CM=8, FLG=0, MTIME=0, XFL=2 (max compression), OS=255 (frame.c:390-401)
      static const unsigned char gz[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 2, 255};
      if (nMax < 10) return ZULTRA_ENCODE_ERR;
      memcpy(p, gz, 10);
      return 10;
   }
   if (nFlags & ZULTRA_FLAG_ZLIB_FRAMING) {
      // RFC 1950: CMF=0x78, FLG: level 3, FDICT if a dictionary is set, FCHECK (frame.c:412-433)
      const bool has_dict = pDict && nDictSize;
      if (nMax < (has_dict ? 6 : 2)) return ZULTRA_ENCODE_ERR;
      unsigned cmf = 0x78, flg = 0xc0 | (has_dict ? 0x20 : 0);
      flg |= (31 - ((cmf << 8 | flg) % 31)) & 0x1f;
      p[0] = (unsigned char)cmf;
      p[1] = (unsigned char)flg;
      if (!has_dict) return 2;
      uint32_t a = adler32_update(1, (const uint8_t *)pDict, (size_t)nDictSize);
      p[2] = (unsigned char)(a >> 24);
      p[3] = (unsigned char)(a >> 16);
      p[4] = (unsigned char)(a >> 8);
      p[5] = (unsigned char)a;
      return 6;
   }
   return 0;
}

extern "C" zultra_frame_checksum_t zultra_frame_init_checksum(const unsigned int nFlags) {
   if (nFlags & ZULTRA_FLAG_GZIP_FRAMING) return 0;
   if (nFlags & ZULTRA_FLAG_ZLIB_FRAMING) return 1;
   return 0;
}

extern "C" zultra_frame_checksum_t zultra_frame_update_checksum(zultra_frame_checksum_t sum, const void *pData, size_t n,
                                                                const unsigned int nFlags) {
   if (nFlags & ZULTRA_FLAG_GZIP_FRAMING) return crc32_update(sum, (const uint8_t *)pData, n);
   if (nFlags & ZULTRA_FLAG_ZLIB_FRAMING) return adler32_update(sum, (const uint8_t *)pData, n);
   return 0;
}

extern "C" int zultra_frame_get_footer_size(const unsigned int nFlags) {
   if (nFlags & ZULTRA_FLAG_GZIP_FRAMING) return 8;
   if (nFlags & ZULTRA_FLAG_ZLIB_FRAMING) return 4;
   return 0;
}

extern "C" int zultra_frame_encode_footer(unsigned char *p, const int nMax, const zultra_frame_checksum_t sum, long long nOriginalSize,
                                          const unsigned int nFlags) {
   if (nFlags & ZULTRA_FLAG_GZIP_FRAMING) {
      if (nMax < 8) return ZULTRA_ENCODE_ERR;
      for (int k = 0; k < 4; k++) p[k] = (unsigned char)(sum >> (8 * k));                                       // CRC32, LE
      for (int k = 0; k < 4; k++) p[4 + k] = (unsigned char)((unsigned long long)nOriginalSize >> (8 * k));   // ISIZE mod 2^32
      return 8;
   }
   if (nFlags & ZULTRA_FLAG_ZLIB_FRAMING) {
      if (nMax < 4) return ZULTRA_ENCODE_ERR;
      for (int k = 0; k < 4; k++) p[k] = (unsigned char)(sum >> (8 * (3 - k)));   // Adler-32, BE
      return 4;
   }
   return 0;
}

// ================================================================================================================
// Dictionary file helper (reference src/dictionary.c:49-104)
// ================================================================================================================

extern "C" zultra_status_t zultra_dictionary_load(const char *name, void **ppData, int *pSize) {
   unsigned char *buf = NULL;
   int n = 0;
   if (name) {
      FILE *f = fopen(name, "rb");
      if (!f) return ZULTRA_ERROR_DICTIONARY;
      buf = (unsigned char *)malloc(HISTORY_SIZE);
      if (!buf) {
         fclose(f);
         return ZULTRA_ERROR_MEMORY;
      }
      fseek(f, 0, SEEK_END);
      long long sz = ftello(f);
      if (sz > HISTORY_SIZE)
         fseek(f, -HISTORY_SIZE, SEEK_END);   // last 32 KiB of the file
      else
         fseek(f, 0, SEEK_SET);
      n = (int)fread(buf, 1, HISTORY_SIZE, f);
      if (n < 0) n = 0;
      fclose(f);
   }
   *ppData = buf;
   *pSize = n;
   return ZULTRA_OK;
}

extern "C" void zultra_dictionary_free(void **ppData) {
   if (ppData && *ppData) {
      free(*ppData);
      *ppData = NULL;
   }
}

// ================================================================================================================
// Stitcher (reference src/libzultra.c:327-398, 414-436; bit writer src/huffman/bitwriter.c:63-98)
// ================================================================================================================

namespace {
struct Sink {
   uint8_t *out;
   size_t cap, pos;
   uint32_t acc, nacc;
   bool overflow;
   bool dry;   // count only (out == NULL): used to plan bit offsets of later shards
   inline void byte(uint8_t b) {
      if (!dry) {
         if (pos < cap)
            out[pos] = b;
         else
            overflow = true;
      }
      pos++;
   }
   inline void bits(uint32_t v, uint32_t n) {   // n <= 16
      acc |= v << nacc;
      nacc += n;
      while (nacc >= 8) {
         byte((uint8_t)acc);
         acc >>= 8;
         nacc -= 8;
      }
   }
   inline void pad() {
      if (nacc) {
         byte((uint8_t)(acc & ((1u << nacc) - 1)));
         acc = 0;
         nacc = 0;
      }
   }
   // append nbits of a phase-0 bit string
   void append(const uint8_t *src, uint64_t nbits) {
      const uint64_t full = nbits >> 3;
      if (dry) {
         pos += full;
         if (nbits & 7) bits(0, (uint32_t)(nbits & 7));
         return;
      }
      if (nacc == 0) {
         size_t room = pos < cap ? cap - pos : 0;
         size_t k = full < room ? (size_t)full : room;
         memcpy(out + pos, src, k);
         if (k < full) overflow = true;
         pos += full;
      }
      else {
         // shift-merge, 8 source bytes per step
         uint64_t i = 0;
         const uint32_t sh = nacc;
         uint64_t carry = acc;
         if (pos + full + 8 <= cap) {
            for (; i + 8 <= full; i += 8) {
               uint64_t v;
               memcpy(&v, src + i, 8);
               uint64_t o = carry | (v << sh);
               memcpy(out + pos, &o, 8);
               pos += 8;
               carry = v >> (64 - sh);
            }
         }
         acc = (uint32_t)carry;
         for (; i < full; i++) bits(src[i], 8);
      }
      if (nbits & 7) bits(src[full] & ((1u << (nbits & 7)) - 1), (uint32_t)(nbits & 7));
   }
};
}   // namespace

extern "C" size_t zultra_hip_stitch(zultra_hip_bitstate_t *state, const zultra_hip_subblock_t *subs, uint32_t nsubs,
                                    const uint8_t *payload, const uint8_t *raw, const uint64_t *raw_off, uint32_t max_block_size,
                                    int final_block, uint8_t *out, size_t out_cap) {
   Sink s{out, out_cap, 0, state->acc, state->nacc, false, out == NULL};
   // capacity of the reference's per-max-block output buffer (libzultra.c:115): exceeding it is ZULTRA_ERROR_DST
   const size_t blockbuf_cap = 1 + (size_t)max_block_size + 5 * ((size_t)max_block_size / 65535 + 1);
   size_t block_base = 0;
   uint32_t cur_block = 0xFFFFFFFFu;

   for (uint32_t k = 0; k < nsubs; k++) {
      const zultra_hip_subblock_t &sb = subs[k];
      if (sb.block != cur_block) {
         cur_block = sb.block;
         block_base = s.pos;   // bitwriter offset restarts at 0 for every max-block, pending bits carry (:427-434)
      }
      const bool last_of_block = (k + 1 == nsubs) || (subs[k + 1].block != sb.block);
      const uint32_t is_final = ((int)sb.block == final_block && last_of_block) ? 1u : 0u;   // :328

      // where the three header bits leave the reference's writer (:329-337)
      const uint32_t c0 = (s.nacc + 3) & 7;
      const size_t o0 = (s.pos - block_base) + ((s.nacc + 3) >> 3);
      if (o0 > blockbuf_cap) return (size_t)-1;
      const uint64_t body_bytes = ((uint64_t)c0 + sb.nbits) >> 3;

      if (!sb.failed && body_bytes <= sb.size && o0 + body_bytes <= blockbuf_cap) {   // :345-347
         s.bits(is_final, 1);
         s.bits(1 + sb.is_dynamic, 2);
         s.append(payload + sb.bits_off, sb.nbits);
      }
      else {
         // stored, pieces of at most 65535 bytes (:350-397)
         const uint8_t *src = s.dry ? NULL : raw + raw_off[sb.block] + sb.start;
         uint32_t rem = sb.size;
         while (rem) {
            const uint32_t piece = rem > 65535 ? 65535 : rem;
            s.bits((rem > 65535) ? 0 : is_final, 1);
            s.bits(0, 2);
            s.pad();
            if ((s.pos - block_base) + 4 + piece > blockbuf_cap) return (size_t)-1;   // :382
            s.byte((uint8_t)(piece & 0xff));
            s.byte((uint8_t)(piece >> 8));
            s.byte((uint8_t)((piece & 0xff) ^ 0xff));
            s.byte((uint8_t)((piece >> 8) ^ 0xff));
            if (!s.dry) {
               if (s.pos + piece <= s.cap)
                  memcpy(s.out + s.pos, src, piece);
               else
                  s.overflow = true;
            }
            s.pos += piece;
            if (!s.dry) src += piece;
            rem -= piece;
         }
      }
   }
   state->acc = s.acc;
   state->nacc = s.nacc;
   return s.overflow ? (size_t)-1 : s.pos;
}

extern "C" size_t zultra_hip_stitch_finish(zultra_hip_bitstate_t *state, uint8_t *out, size_t out_cap) {
   if (!state->nacc) return 0;
   if (out_cap < 1) return (size_t)-1;
   out[0] = (uint8_t)(state->acc & ((1u << state->nacc) - 1));   // libzultra.c:414-417
   state->acc = 0;
   state->nacc = 0;
   return 1;
}

// ================================================================================================================
// Devices, cached contexts, verification
// ================================================================================================================

static int g_device = -1;
static std::mutex g_ctx_mutex;
struct CachedCtx {
   zultra_hip_ctx_t *ctx;
   int device;
   uint32_t max_block, max_blocks;
};
static std::vector<CachedCtx> g_ctx_pool;   // contexts released by finished streams, reused by later ones

static int zh_pick_device() { return g_device >= 0 ? g_device : zh_env("ZULTRA_HIP_DEVICE", 0); }

extern "C" void zultra_set_device(int nDevice) { g_device = nDevice; }

// The devices zultra_memory_compress spreads an input over: zultra_set_devices, else ZULTRA_HIP_DEVICES="0,1,2,..." (a device may be
// named more than once: "0,0" = two contexts on device 0, the kernels of one batch next to the transfers of another), else none.
static std::vector<int> g_devices;
extern "C" int zultra_set_devices(const int *pDevices, int nDevices) {
   std::lock_guard<std::mutex> lk(g_ctx_mutex);
   g_devices.clear();
   const int have = zultra_hip_device_count();
   for (int i = 0; i < nDevices; i++) {
      if (pDevices[i] < 0 || pDevices[i] >= have) {
         g_devices.clear();
         return -1;
      }
      g_devices.push_back(pDevices[i]);
   }
   return nDevices;
}
static std::vector<int> zh_pick_devices() {
   {
      std::lock_guard<std::mutex> lk(g_ctx_mutex);
      if (!g_devices.empty()) return g_devices;
   }
   std::vector<int> v;
   const char *e = getenv("ZULTRA_HIP_DEVICES");
   if (e) {
      const int have = zultra_hip_device_count();
      for (const char *p = e; *p;) {
         char *end = NULL;
         const long d = strtol(p, &end, 10);
         if (end == p) break;
         if (d >= 0 && d < have) v.push_back((int)d);
         p = (*end == ',') ? end + 1 : end;
      }
   }
   return v;
}

// input bytes -> pinned staging, split over a few threads from 2 * piece bytes on. Shared with the device layer (zh_device.hip), not exported.
ZH_HIDDEN void zh_threaded_copy(uint8_t *dst, const uint8_t *src, size_t n, size_t piece) {
   if (n < 2 * piece) {
      memcpy(dst, src, n);
      return;
   }
   const size_t nt = n / piece < 4 ? n / piece : 4;
   std::vector<std::thread> th;
   size_t started = 1;   // pieces 1 .. started - 1 have a thread; nothing thrown here may cross the C ABI (extern "C" callers end in std::terminate)
   try {
      th.reserve(nt);
      for (; started < nt; started++) th.emplace_back([=] { memcpy(dst + n * started / nt, src + n * started / nt, n * (started + 1) / nt - n * started / nt); });
   } catch (...) {
   }
   memcpy(dst, src, n / nt);
   if (started < nt) memcpy(dst + n * started / nt, src + n * started / nt, n - n * started / nt);   // (no thread for the rest: copied here)
   for (auto &t : th) t.join();
}

// ---- verification (libzultra.h: zultra_set_verify) ------------------------------------------------------------------------------------------
static std::atomic<int> g_verify{-1};   // -1: not set by the caller, the environment decides
static std::atomic<unsigned long long> g_verified_bytes{0};
extern "C" void zultra_set_verify(int nEnable) { g_verify.store(nEnable ? 1 : 0); }
extern "C" unsigned long long zultra_verified_bytes(void) { return g_verified_bytes.load(); }
static bool zh_verify_on() {
   const int v = g_verify.load();
   return v >= 0 ? v != 0 : zh_env("ZULTRA_HIP_VERIFY", 0) != 0;
}
// The batch the context has just stitched, inflated on its device and compared with its input. false: a mismatch (one line on stderr) or an error.
static bool zh_verify_stitched(zultra_hip_ctx_t *c) {
   zultra_hip_verify_t r;
   const int rc = zultra_hip_verify_device(c, &r);
   if (rc == 0) {
      g_verified_bytes.fetch_add(r.verified_bytes);
      return true;
   }
   if (rc == 1)
      fprintf(stderr, "zultra: verification failed: %u sub-block(s) do not inflate to the input; first: sub-block %u, reason %u, max-block %u, input offset %llu, stream bit %llu\n",
              r.bad_subblocks, r.first_bad, r.reason, r.block, (unsigned long long)r.input_off, (unsigned long long)r.stream_bit);
   else
      fprintf(stderr, "zultra: verification could not run: %s\n", zultra_hip_last_error(c));
   return false;
}

static zultra_hip_ctx_t *ctx_acquire_on(int dev, uint32_t bs, uint32_t want_blocks) {
   std::lock_guard<std::mutex> lk(g_ctx_mutex);
   for (size_t i = 0; i < g_ctx_pool.size(); i++) {
      if (g_ctx_pool[i].device == dev && g_ctx_pool[i].max_block == bs && g_ctx_pool[i].max_blocks >= want_blocks) {
         zultra_hip_ctx_t *c = g_ctx_pool[i].ctx;
         g_ctx_pool.erase(g_ctx_pool.begin() + (long)i);
         return c;
      }
   }
   // a smaller cached context of the same geometry would only waste memory next to the new one
   for (size_t i = 0; i < g_ctx_pool.size();) {
      if (g_ctx_pool[i].device == dev && g_ctx_pool[i].max_block == bs) {
         zultra_hip_destroy(g_ctx_pool[i].ctx);
         g_ctx_pool.erase(g_ctx_pool.begin() + (long)i);
      }
      else
         i++;
   }
   return zultra_hip_create(dev, bs, want_blocks);
}

// A finished stream's context goes back under what the CONTEXT says it is (device, block size, capacity) — not under what the
// stream asked for or what zultra_set_device says now.
static void ctx_release(zultra_hip_ctx_t *c) {
   if (!c) return;
   if (zh_env("ZULTRA_HIP_CACHE", 1) == 0) {
      zultra_hip_destroy(c);
      return;
   }
   CachedCtx cc;
   cc.ctx = c;
   zultra_hip_ctx_info(c, &cc.device, &cc.max_block, &cc.max_blocks, NULL);
   std::lock_guard<std::mutex> lk(g_ctx_mutex);
   size_t same = 0, first_same = 0;   // at most two kept per device
   for (size_t i = g_ctx_pool.size(); i-- > 0;)
      if (g_ctx_pool[i].device == cc.device) {
         same++;
         first_same = i;
      }
   if (same >= 2) {
      zultra_hip_destroy(g_ctx_pool[first_same].ctx);
      g_ctx_pool.erase(g_ctx_pool.begin() + (long)first_same);
   }
   g_ctx_pool.push_back(cc);
}

extern "C" int zultra_release_cached_contexts(void) {
   std::lock_guard<std::mutex> lk(g_ctx_mutex);
   const int n = (int)g_ctx_pool.size();
   for (size_t i = 0; i < g_ctx_pool.size(); i++) zultra_hip_destroy(g_ctx_pool[i].ctx);
   g_ctx_pool.clear();
   return n;
}

// The max-blocks a context on `device` gets when `want` are asked for (0: a stream, which does not know its input, stages 64 MiB): at most 8192, at
// most ZULTRA_HIP_BATCH_BLOCKS where that is set (2 at the least; a negative value counts as not set), and no more than 24 GiB of device memory
// (MI355X has 288 GB), sized from the layout the context will really allocate.
static uint32_t ctx_blocks(int device, uint32_t bs, uint64_t want) {
   const int knob = zh_env("ZULTRA_HIP_BATCH_BLOCKS", -1);
   uint64_t n = want;
   if (knob >= 0 || !want) {
      const uint64_t k = zh_max64(knob >= 0 ? (uint64_t)knob : (64u << 20) / bs, 2);
      n = want ? zh_min64(want, k) : k;
   }
   n = zh_min64(n, 8192);
   while (n > 1 && (uint64_t)zultra_hip_context_bytes_on(device, bs, (uint32_t)n) > (24ull << 30)) n -= (n + 7) / 8;
   return (uint32_t)n;
}

// ================================================================================================================
// One batch of max-blocks (reference src/libzultra.c:250-253, 279, 287-303, 327-398, 414-436): what a batch of the stream API and a job of
// zultra_memory_compress's lanes both do, stated once
// ================================================================================================================

// Descriptors of `count` max-blocks of `bs` bytes (the last one `last_n`) that lie one behind the other after `hist` bytes of history: the first
// block's history is those bytes, every later block's the 32 KiB in front of it (blocks are >= 32 KiB unless last).
static void batch_describe(zultra_hip_block_t *blocks, size_t hist, uint32_t bs, size_t count, uint32_t last_n) {
   for (size_t b = 0; b < count; b++) {
      const uint32_t prev = b == 0 ? (uint32_t)hist : (uint32_t)HISTORY_SIZE;
      blocks[b].win_off = (uint64_t)hist + (uint64_t)b * bs - prev;
      blocks[b].prev = prev;
      blocks[b].n = b + 1 == count ? last_n : bs;
   }
}

// A preset dictionary is the pre-filled history of a stream's first max-block (libzultra.c:250-253): its last 32 KiB, or all of it
static const uint8_t *dict_history(const void *dict, int dict_size, size_t *hist) {
   *hist = dict_size > HISTORY_SIZE ? (size_t)HISTORY_SIZE : (size_t)dict_size;
   return (const uint8_t *)dict + ((size_t)dict_size - *hist);
}

// Checksum once per max-block over its bytes (libzultra.c:279): both kinds are computed on the device next to the compression and folded into the
// running checksum here. `crc` has room for one value per max-block, `adler_parts` for two.
static bool batch_fold_checksums(zultra_hip_ctx_t *c, unsigned flags, const zultra_hip_block_t *blocks, uint32_t count, uint32_t *crc, uint32_t *adler_parts,
                                 zultra_frame_checksum_t *sum) {
   if (flags & ZULTRA_FLAG_GZIP_FRAMING) {
      if (zultra_hip_block_crc32(c, crc) != (int)count) return false;
      for (uint32_t b = 0; b < count; b++) *sum = zultra_crc32_append(*sum, crc[b], blocks[b].n);
   }
   else if (flags & ZULTRA_FLAG_ZLIB_FRAMING) {
      if (zultra_hip_block_adler32(c, adler_parts) != (int)count) return false;
      for (uint32_t b = 0; b < count; b++) *sum = zultra_adler32_append(*sum, adler_parts[2 * b], adler_parts[2 * b + 1], blocks[b].n);
   }
   return true;
}

// Finish the context's batch on the device at the phase `bit` has reached: descriptors -> plan, the bits moved by a kernel (nothing is launched where the
// stitch went out with the batch, zultra_hip_stitch_with_batch), verified there if asked, one D2H of the finished bytes into pinned memory — *dst of
// dst_cap bytes, or, where *dst is NULL, the context's output staging grown to the batch, which *dst then names. The pending bits of the batches before
// go into byte 0; *whole bytes are the caller's to hand out; a trailing partial byte stays pending in `bit` for the next batch, the final batch's is
// already zero padded (libzultra.c:414-417). ZULTRA_ERROR_DST where the reference fails with it (the stitch's -2) and where dst_cap is too little.
static zultra_status_t batch_finish(zultra_hip_ctx_t *c, zultra_hip_bitstate_t *bit, int final_block, uint8_t **dst, size_t dst_cap, size_t *whole) {
   const uint32_t pending = bit->acc & ((1u << bit->nacc) - 1);
   uint64_t end_bit = 0;
   const int rc = zultra_hip_stitch_device(c, bit, final_block, &end_bit);
   if (rc == -2) return ZULTRA_ERROR_DST;
   if (rc != 0) return ZULTRA_ERROR_COMPRESSION;
   if (zh_verify_on() && !zh_verify_stitched(c)) return ZULTRA_ERROR_COMPRESSION;
   const size_t total = (size_t)((end_bit + 7) >> 3);
   if (!*dst) {
      if (!(*dst = (uint8_t *)zultra_hip_staging(c, 1, total + 16))) return ZULTRA_ERROR_COMPRESSION;
   }
   else if (total > dst_cap)
      return ZULTRA_ERROR_DST;
   if (zultra_hip_stream_read(c, *dst, 0, total) != 0) return ZULTRA_ERROR_COMPRESSION;
   (*dst)[0] |= (uint8_t)pending;
   if (final_block >= 0) {
      *whole = total;
      bit->acc = bit->nacc = 0;
   }
   else {
      *whole = (size_t)(end_bit >> 3);
      bit->acc = (end_bit & 7) ? (*dst)[*whole] : 0;
   }
   return ZULTRA_OK;
}

// ================================================================================================================
// Streaming API (reference src/libzultra.c:82-565)
// ================================================================================================================

enum StreamState : unsigned {   // bits of _zultra_compressor_s::state
   ST_HAS_DICTIONARY = 1,
   ST_HEADER_EMITTED = 2,
   ST_FINALIZED = 4,
   ST_FOOTER_EMITTED = 8,
   ST_STREAM_ENDED = 16,
};

struct _zultra_compressor_s {
   unsigned flags = 0;
   uint32_t max_block = 0;
   uint32_t batch_blocks = 0;       // max-blocks per device batch
   uint64_t flush_bytes = 0;        // staged full max-blocks of this many bytes are compressed when a call's input is used up (0: only when the staging area is full)
   const void *dict = NULL;
   int dict_size = 0;
   unsigned state = 0;              // StreamState bits

   zultra_hip_ctx_t *hip = NULL;
   zultra_hip_bitstate_t bitstate = {};

   uint8_t *in = NULL;              // [32 KiB history][batch_blocks * max_block]
   size_t in_bytes = 0;             // input bytes staged after the history area
   int prev = 0;                    // valid history bytes (end-aligned in the history area)

   uint8_t *out = NULL;             // stitched bytes of the last batch
   size_t out_cap = 0, out_pos = 0, out_pending = 0;

   unsigned char frame[16];
   size_t frame_pos = 0, frame_pending = 0;

   // per max-block of a batch, batch_blocks entries each, from the caller's allocator (libzultra.c:94-147: every buffer of a stream
   // comes from zalloc; what does not here is the device context — device memory and pinned staging — which belongs to the backend)
   zultra_hip_block_t *blocks = NULL;
   uint64_t *raw_off = NULL;
   uint32_t *crc = NULL;
   uint32_t *adler_parts = NULL;    // two per max-block
   bool host_stitch = false;        // ZULTRA_HIP_HOST_STITCH=1: stitch on the host (A/B checking)
};

static void *default_zalloc(void *, unsigned int items, unsigned int size) { return malloc((size_t)items * size); }
static void default_zfree(void *, void *p) { free(p); }

// want_blocks: the max-blocks of the input where the whole of it is at hand, 0 for a stream (ctx_blocks)
static zultra_status_t stream_init_sized(zultra_stream_t *s, unsigned flags, unsigned bs_in, uint64_t want_blocks) {
   const uint32_t bs = zh_clamp_block(bs_in);
   if (!s->zalloc) s->zalloc = default_zalloc;
   if (!s->zfree) s->zfree = default_zfree;
   s->adler = 0;
   s->state = NULL;

   zultra_compressor_t *c = (zultra_compressor_t *)s->zalloc(s->opaque, 1, (unsigned)sizeof(zultra_compressor_t));
   if (!c) return ZULTRA_ERROR_MEMORY;
   new (c) zultra_compressor_t();   // (the object itself is the caller's memory like its arrays; the member initialisers above are its start state)
   s->state = c;
   c->flags = flags;
   c->max_block = bs;
   c->host_stitch = zh_env("ZULTRA_HIP_HOST_STITCH", 0) != 0;
   c->flush_bytes = zh_env64("ZULTRA_HIP_FLUSH_BYTES", 4ull << 20);
   const uint32_t batch_blocks = c->batch_blocks = ctx_blocks(zh_pick_device(), bs, want_blocks);

   c->blocks = (zultra_hip_block_t *)s->zalloc(s->opaque, batch_blocks, (unsigned)sizeof(zultra_hip_block_t));
   c->raw_off = (uint64_t *)s->zalloc(s->opaque, batch_blocks, (unsigned)sizeof(uint64_t));
   c->crc = (uint32_t *)s->zalloc(s->opaque, batch_blocks, (unsigned)sizeof(uint32_t));
   c->adler_parts = (uint32_t *)s->zalloc(s->opaque, 2 * batch_blocks, (unsigned)sizeof(uint32_t));
   if (c->blocks && c->raw_off && c->crc && c->adler_parts) c->hip = ctx_acquire_on(zh_pick_device(), bs, batch_blocks);
   if (c->hip) {
      // worst case per max-block: all sub-blocks stored (libzultra.c:576-587)
      c->out_cap = (size_t)batch_blocks * ((size_t)bs + 6 * 64 + 16) + 16;
      // staging lives in pinned memory owned by the (pooled) device context: it survives this stream and is reused by the next
      c->in = (uint8_t *)zultra_hip_staging(c->hip, 0, (size_t)HISTORY_SIZE + (size_t)batch_blocks * bs);
      c->out = (uint8_t *)zultra_hip_staging(c->hip, 1, c->out_cap);
   }
   if (!c->in || !c->out) {   // an array, or no usable HIP device / device memory (there is no CPU path), or the staging
      zultra_stream_end(s);
      return ZULTRA_ERROR_MEMORY;
   }
   return ZULTRA_OK;
}

extern "C" zultra_status_t zultra_stream_init(zultra_stream_t *s, const unsigned int nFlags, unsigned int nMaxBlockSize) {
   return stream_init_sized(s, nFlags, nMaxBlockSize, 0);
}

extern "C" zultra_status_t zultra_stream_set_dictionary(zultra_stream_t *s, const void *pDict, const int nDictSize) {
   zultra_compressor_t *c = s->state;
   if (c && c->state == 0) {   // only before the first compress call (libzultra.c:180)
      c->dict = pDict;
      c->dict_size = nDictSize;
      c->state |= ST_HAS_DICTIONARY;
      return ZULTRA_OK;
   }
   return ZULTRA_ERROR_COMPRESSION;
}

extern "C" void zultra_stream_end(zultra_stream_t *s) {
   if (s->state && s->zfree) {
      zultra_compressor_t *c = s->state;
      ctx_release(c->hip);
      /* c->in / c->out belong to the device context */
      if (c->blocks) s->zfree(s->opaque, c->blocks);
      if (c->raw_off) s->zfree(s->opaque, c->raw_off);
      if (c->crc) s->zfree(s->opaque, c->crc);
      if (c->adler_parts) s->zfree(s->opaque, c->adler_parts);
      c->~zultra_compressor_t();
      s->zfree(s->opaque, c);
      s->state = NULL;
   }
}

// The output pump: pending bytes of `buf` (frame bytes, a batch's bytes) go to next_out as far as there is room
static void pump_out(zultra_stream_t *s, const uint8_t *buf, size_t *pos, size_t *pending) {
   const size_t k = s->avail_out < *pending ? s->avail_out : *pending;
   if (!k) return;
   memcpy(s->next_out, buf + *pos, k);
   *pos += k;
   *pending -= k;
   s->next_out += k;
   s->avail_out -= k;
   s->total_out += k;
}

// Compress `count` max-blocks staged at c->in + HISTORY (the last one `last_n` bytes long).
static zultra_status_t compress_staged(zultra_stream_t *s, zultra_compressor_t *c, uint32_t count, uint32_t last_n, bool final_last) {
   const uint32_t bs = c->max_block;
   if (count > c->batch_blocks) return ZULTRA_ERROR_COMPRESSION;
   const int final_block = final_last ? (int)count - 1 : -1;
   const size_t consumed = (size_t)(count - 1) * bs + last_n;
   batch_describe(c->blocks, (size_t)c->prev, bs, count, last_n);
   // the phase this batch starts at is what the batches before it left (libzultra.c:327-398): its stitch goes out with its kernels
   if (!c->host_stitch) (void)zultra_hip_stitch_with_batch(c->hip, 1, c->bitstate.nacc, final_block);
   if (zultra_hip_compress_blocks(c->hip, c->in + HISTORY_SIZE - c->prev, (size_t)c->prev + consumed, 0, c->blocks, count) <= 0) return ZULTRA_ERROR_COMPRESSION;
   if (!batch_fold_checksums(c->hip, c->flags, c->blocks, count, c->crc, c->adler_parts, &s->adler)) return ZULTRA_ERROR_COMPRESSION;

   size_t w = 0;
   if (!c->host_stitch) {
      uint8_t *out = c->out;
      const zultra_status_t st = batch_finish(c->hip, &c->bitstate, final_block, &out, c->out_cap, &w);
      if (st != ZULTRA_OK) return st;
   }
   else {
      if (zh_verify_on()) {
         // the host stitcher's bytes never reach the device: the same batch is stitched there too, from the same phase, and that stream is checked
         zultra_hip_bitstate_t dev_state = c->bitstate;
         uint64_t end_bit = 0;
         const int rc = zultra_hip_stitch_device(c->hip, &dev_state, final_block, &end_bit);
         if (rc == -2) return ZULTRA_ERROR_DST;
         if (rc != 0 || !zh_verify_stitched(c->hip)) return ZULTRA_ERROR_COMPRESSION;
      }
      uint32_t cnt = 0;
      const zultra_hip_subblock_t *subs = zultra_hip_subblocks(c->hip, &cnt);
      size_t psize = 0;
      const uint8_t *payload = zultra_hip_payload(c->hip, &psize);
      for (uint32_t b = 0; b < count; b++) c->raw_off[b] = (uint64_t)b * bs;
      w = zultra_hip_stitch(&c->bitstate, subs, cnt, payload, c->in + HISTORY_SIZE, c->raw_off, bs, final_block, c->out, c->out_cap);
      if (w == (size_t)-1) return ZULTRA_ERROR_DST;
      if (final_last) {
         size_t f = zultra_hip_stitch_finish(&c->bitstate, c->out + w, c->out_cap - w);
         if (f == (size_t)-1) return ZULTRA_ERROR_DST;
         w += f;
      }
   }
   if (final_last) c->state |= ST_FINALIZED;
   c->out_pos = 0;
   c->out_pending = w;

   // slide: the last <= 32 KiB just compressed become the history of what follows (libzultra.c:406-412)
   size_t keep = consumed < (size_t)HISTORY_SIZE ? consumed : (size_t)HISTORY_SIZE;
   if (consumed < (size_t)HISTORY_SIZE) {
      // (only possible for a last, short block; kept for symmetry) old history stays in front
      size_t old = (size_t)c->prev;
      if (old + consumed > (size_t)HISTORY_SIZE) old = (size_t)HISTORY_SIZE - consumed;
      memmove(c->in + HISTORY_SIZE - keep - old, c->in + HISTORY_SIZE - old, old);
      memmove(c->in + HISTORY_SIZE - keep, c->in + HISTORY_SIZE, keep);
      c->prev = (int)(old + keep);
   }
   else {
      memmove(c->in, c->in + HISTORY_SIZE + consumed - HISTORY_SIZE, HISTORY_SIZE);
      c->prev = HISTORY_SIZE;
   }
   const size_t left = c->in_bytes - consumed;
   if (left) memmove(c->in + HISTORY_SIZE, c->in + HISTORY_SIZE + consumed, left);
   c->in_bytes = left;
   c->dict_size = 0;
   return ZULTRA_OK;
}

extern "C" zultra_status_t zultra_stream_compress(zultra_stream_t *s, const int nDoFinalize) {
   zultra_compressor_t *c = s->state;
   zultra_status_t err = ZULTRA_OK;
   if (!c) return ZULTRA_ERROR_COMPRESSION;
   if (c->state & ST_STREAM_ENDED) return ZULTRA_ERROR_COMPRESSION;
   const uint32_t bs = c->max_block;

   do {
      if (!(c->state & ST_HEADER_EMITTED)) {
         c->state |= ST_HEADER_EMITTED;
         int h = zultra_frame_encode_header(c->frame, 16, c->flags, c->dict, c->dict_size);
         if (h < 0)
            err = ZULTRA_ERROR_COMPRESSION;
         else {
            c->frame_pos = 0;
            c->frame_pending = (size_t)h;
         }
         s->adler = zultra_frame_init_checksum(c->flags);
      }
      if (!err) pump_out(s, c->frame, &c->frame_pos, &c->frame_pending);

      if (!err && !c->prev && c->dict_size && c->dict && c->in_bytes == 0) {
         size_t d = 0;
         const uint8_t *tail = dict_history(c->dict, c->dict_size, &d);
         memcpy(c->in + HISTORY_SIZE - d, tail, d);
         c->prev = (int)d;
      }

      if (!err && !c->frame_pending && !c->out_pending) {
         const size_t cap = (size_t)c->batch_blocks * bs;
         size_t take = s->avail_in;
         if (take > cap - c->in_bytes) take = cap - c->in_bytes;
         memcpy(c->in + HISTORY_SIZE + c->in_bytes, s->next_in, take);
         s->next_in += take;
         s->avail_in -= take;
         s->total_in += take;
         c->in_bytes += take;

         // which staged max-blocks may be compressed now (libzultra.c:269): a full block needs more input behind
         // it, or ZULTRA_FINALIZE; a partial block needs ZULTRA_FINALIZE
         const uint32_t full = (uint32_t)(c->in_bytes / bs);
         const uint32_t rem = (uint32_t)(c->in_bytes % bs);
         uint32_t count = 0, last_n = bs;
         bool final_last = false;
         if (nDoFinalize) {
            count = full + (rem ? 1 : 0);
            if (rem) last_n = rem;
            final_last = (s->avail_in == 0);
         }
         else if (full) {
            // A full max-block may be compressed once input beyond it has been seen (libzultra.c:269). Nothing obliges us to do it
            // at once: blocks are kept until the staging area is full, so that a caller feeding small chunks (the reference's
            // CLI reads 16 KiB at a time) still gets device batches of many max-blocks instead of one launch sequence per block.
            // Neither may a caller that pipes the output on wait for it for long: once the caller has nothing more to give in this call and
            // `flush_bytes` of full blocks are staged (4 MiB unless ZULTRA_HIP_FLUSH_BYTES says otherwise; the reference publishes after every
            // max-block, libzultra.c:424-462), they go to the device. A caller that hands over tens of MiB at once still fills the whole
            // staging area (64 MiB) first: the big batches are for those who have the data.
            const uint32_t ready = (rem || s->avail_in) ? full : full - 1;
            if (c->in_bytes >= cap || (ready >= c->batch_blocks) || (c->flush_bytes && s->avail_in == 0 && (uint64_t)ready * bs >= c->flush_bytes)) count = ready;
         }
         if (count) err = compress_staged(s, c, count, last_n, final_last && count > 0);
      }

      if (!err && !c->frame_pending) pump_out(s, c->out, &c->out_pos, &c->out_pending);

      if (!err && !c->frame_pending && !c->out_pending && (c->state & ST_FINALIZED) && !(c->state & ST_FOOTER_EMITTED)) {
         int f = zultra_frame_encode_footer(c->frame, 16, s->adler, (long long)s->total_in, c->flags);
         if (f < 0)
            err = ZULTRA_ERROR_COMPRESSION;
         else {
            c->state = (c->state | ST_FOOTER_EMITTED) & ~(unsigned)ST_FINALIZED;
            c->frame_pos = 0;
            c->frame_pending = (size_t)f;
         }
      }
      if (!err) pump_out(s, c->frame, &c->frame_pos, &c->frame_pending);
   } while (!err && s->avail_in && s->avail_out);

   if (err) return err;
   if ((c->state & ST_FOOTER_EMITTED) && !(c->state & ST_STREAM_ENDED) && !c->frame_pending) {
      c->state |= ST_STREAM_ENDED;
      return ZULTRA_STREAM_END;
   }
   return ZULTRA_OK;
}

// ================================================================================================================
// In-memory API (reference src/libzultra.c:576-619)
// ================================================================================================================

extern "C" size_t zultra_memory_bound(size_t nInputSize, const unsigned int nFlags, unsigned int nMaxBlockSize) {
   const size_t bs = zh_clamp_block(nMaxBlockSize);
   return (size_t)zultra_frame_get_header_size(nFlags, NULL, 0) + ((nInputSize + (bs - 1)) / bs) * (1 + 4 + 1) * 64 + nInputSize + 1 +
          (size_t)zultra_frame_get_footer_size(nFlags);
}

// ---- in-memory compression over several device contexts ("lanes") ---------------------------------------------------------------
// The reference's zultra_memory_compress (libzultra.c:601-619) is one stream; here the whole input is at hand, and max-blocks only
// need the 32 KiB in front of them: the input is cut into contiguous *jobs* of max-blocks, job j goes to lane j % lanes — a lane = a
// device context on one of the devices of ZULTRA_HIP_DEVICES / zultra_set_devices, with a host thread of its own that stages the job's
// bytes into the context's pinned memory and runs the batch (upload + kernels). What depends on the bit phase the stream has reached —
// BFINAL / BTYPE bits, stored fallback, bit carry (libzultra.c:327-398,414-436) — is the stitch, and that is done by the calling
// thread job by job in stream order, on the job's own device, as soon as the job's batch is done; the stitched bytes go to pOut
// while the lanes are at their next jobs. Same bytes as the one-stream path: both cut max-blocks at multiples of the block size.
namespace {
enum class JobState { Waiting, BatchDone, Stitched };   // Stitched: and read out — the lane's context is free for the lane's next job
struct MemJob {
   size_t first, bytes;                       // the job's input: `bytes` from offset `first`
   const uint8_t *hist_src;                   // history of its first max-block: the `hist` bytes of input in front of it, or the preset dictionary's
   size_t hist;
   std::vector<zultra_hip_block_t> blocks;   // its max-blocks: the lane compresses them, the stitching thread folds their checksums
   JobState state = JobState::Waiting;
};
struct MemLanes {
   const uint8_t *in = NULL;
   uint32_t bs = 0;
   std::vector<MemJob> jobs;
   std::vector<zultra_hip_ctx_t *> ctx;   // one per lane
   std::vector<std::thread> threads;
   std::mutex m;
   std::condition_variable cv;
   bool failed = false;

   void fail() {
      {
         std::lock_guard<std::mutex> lk(m);
         failed = true;
      }
      cv.notify_all();
   }
   void set(MemJob &J, JobState s) {
      {
         std::lock_guard<std::mutex> lk(m);
         J.state = s;
      }
      cv.notify_all();
   }
   // until J is in state s (J == NULL: nothing to wait for); false: the call has failed meanwhile
   bool wait(const MemJob *J, JobState s) {
      std::unique_lock<std::mutex> lk(m);
      cv.wait(lk, [&] { return failed || !J || J->state == s; });
      return !failed;
   }
   void lane(size_t l);
   // the one exit: whoever still waits gives up, every thread is joined, every context goes back
   ~MemLanes() {
      fail();
      for (auto &t : threads) t.join();
      for (auto *c : ctx) ctx_release(c);
   }
};

void MemLanes::lane(size_t l) try {
   zultra_hip_ctx_t *c = ctx[l];
   for (size_t j = l; j < jobs.size(); j += ctx.size()) {
      MemJob &J = jobs[j];
      // the lane's previous job must have left the context (stitched and read out)
      if (!wait(j >= ctx.size() ? &jobs[j - ctx.size()] : NULL, JobState::Stitched)) return;
      // The job's windows are contiguous in the caller's buffer — unless its history is the preset dictionary — and are handed over
      // as they are: the device layer stages and uploads them run by run (zultra_hip_compress_blocks, data_on_device == 2).
      const bool in_place = J.hist_src + J.hist == in + J.first;
      uint8_t *stage = in_place ? (uint8_t *)J.hist_src : (uint8_t *)zultra_hip_staging(c, 0, (size_t)HISTORY_SIZE + J.blocks.size() * bs);
      if (stage && !in_place) {
         memcpy(stage, J.hist_src, J.hist);
         zh_threaded_copy(stage + J.hist, in + J.first, J.bytes, 16u << 20);   // (what a lane's first job waits for)
      }
      // the stream's first job starts at phase 0: its stitch goes out with its kernels (the later jobs' phases are known when the jobs before them are stitched)
      if (stage && j == 0) (void)zultra_hip_stitch_with_batch(c, 1, 0, jobs.size() == 1 ? (int)J.blocks.size() - 1 : -1);
      if (!stage || zultra_hip_compress_blocks(c, stage, J.hist + J.bytes, in_place ? 2 : 0, J.blocks.data(), (uint32_t)J.blocks.size()) <= 0) {
         fail();
         return;
      }
      set(J, JobState::BatchDone);
   }
} catch (...) {   // (std::system_error from a lock: the call fails, the process does not)
   fail();
}
}   // namespace

// Nothing thrown in here crosses the C ABI (std::bad_alloc from the vectors, std::system_error from a thread that cannot start): the call fails, and
// ~MemLanes has joined what was started and released the contexts before the handler runs.
static size_t memory_compress_lanes(const unsigned char *pIn, size_t nIn, unsigned char *pOut, size_t nOutCap, const unsigned int nFlags, uint32_t bs,
                                    const void *pDict, int nDictSize, const std::vector<int> &devices) try {
   // jobs: as few as there are lanes when the input fits that way, else batches of the size a one-stream call would use
   const size_t total_blocks = (nIn + bs - 1) / bs;
   size_t per = (total_blocks + devices.size() - 1) / devices.size();
   for (int dv : devices) per = ctx_blocks(dv, bs, per);   // (the listed devices need not be alike: a job must fit the smallest budget)
   MemLanes M;
   M.in = pIn;
   M.bs = bs;
   for (size_t b = 0; b < total_blocks; b += per) {
      const size_t nb = total_blocks - b < per ? total_blocks - b : per, first = b * bs, bytes = nb * bs < nIn - first ? nb * bs : nIn - first;
      size_t hist = first < (size_t)HISTORY_SIZE ? first : (size_t)HISTORY_SIZE;
      const uint8_t *hist_src = pIn + first - hist;
      if (b == 0 && pDict && nDictSize > 0) hist_src = dict_history(pDict, nDictSize, &hist);
      M.jobs.push_back(MemJob{first, bytes, hist_src, hist, std::vector<zultra_hip_block_t>(nb)});
      batch_describe(M.jobs.back().blocks.data(), hist, bs, nb, (uint32_t)(bytes - (nb - 1) * bs));
   }
   // a lane whose context cannot be had (a second large context on a device listed twice, a busy or smaller device) is left out: the
   // jobs go round the lanes that exist; none at all is the only failure
   for (size_t l = 0; l < devices.size() && l < M.jobs.size(); l++) {
      zultra_hip_ctx_t *c = ctx_acquire_on(devices[l], bs, (uint32_t)per);
      if (c) M.ctx.push_back(c);
   }
   const size_t lanes = M.ctx.size();
   if (!lanes) return (size_t)-1;
   // (one lane with one job — a call on a few max-blocks, where 50 us of thread start-up and wake-ups count — runs on the calling thread)
   if (lanes == 1 && M.jobs.size() == 1)
      M.lane(0);
   else {
      M.threads.reserve(lanes);
      for (size_t l = 0; l < lanes; l++) M.threads.emplace_back(&MemLanes::lane, &M, l);
   }

   unsigned char frame[16];
   const int h = zultra_frame_encode_header(frame, 16, nFlags, pDict, nDictSize);
   if (h < 0 || (size_t)h > nOutCap) return (size_t)-1;
   memcpy(pOut, frame, (size_t)h);
   size_t w = (size_t)h;
   zultra_frame_checksum_t sum = zultra_frame_init_checksum(nFlags);
   zultra_hip_bitstate_t bit = {};
   std::vector<uint32_t> parts(2 * per);
   for (size_t j = 0; j < M.jobs.size(); j++) {
      MemJob &J = M.jobs[j];
      zultra_hip_ctx_t *c = M.ctx[j % lanes];
      const uint32_t nb = (uint32_t)J.blocks.size();
      uint8_t *bytes = NULL;   // (the context's output staging)
      size_t whole = 0;
      if (!M.wait(&J, JobState::BatchDone) || !batch_fold_checksums(c, nFlags, J.blocks.data(), nb, parts.data(), parts.data(), &sum) ||
          batch_finish(c, &bit, j + 1 == M.jobs.size() ? (int)nb - 1 : -1, &bytes, 0, &whole) != ZULTRA_OK || w + whole > nOutCap)
         return (size_t)-1;
      memcpy(pOut + w, bytes, whole);
      w += whole;
      M.set(J, JobState::Stitched);
   }
   const int f = zultra_frame_encode_footer(frame, 16, sum, (long long)nIn, nFlags);
   if (f < 0 || w + (size_t)f > nOutCap) return (size_t)-1;
   memcpy(pOut + w, frame, (size_t)f);
   return w + (size_t)f;
} catch (...) {
   return (size_t)-1;
}

extern "C" size_t zultra_memory_compress_dict(const unsigned char *pIn, size_t nIn, unsigned char *pOut, size_t nOutCap,
                                              const unsigned int nFlags, unsigned int nMaxBlockSize, const void *pDict, int nDictSize) {
   zultra_stream_t strm;
   memset(&strm, 0, sizeof(strm));
   const uint32_t bs = zh_clamp_block(nMaxBlockSize);
   const size_t nblocks = (nIn + bs - 1) / bs;
   // The whole input is at hand: shards of max-blocks over the devices asked for (ZULTRA_HIP_DEVICES / zultra_set_devices; "0,0" = two
   // contexts on device 0), at least two max-blocks per lane — or one lane on the one device, its batch staged and uploaded run by run.
   // (ZULTRA_HIP_MEMORY_LANES=0: through the stream API instead, as the reference does, libzultra.c:601-619.)
   try {
      std::vector<int> devs = zh_pick_devices();
      if (devs.empty())
         for (int l = zh_env("ZULTRA_HIP_MEMORY_LANES", 1); l > 0; l--) devs.push_back(zh_pick_device());
      while (devs.size() > 1 && nblocks < 2 * devs.size()) devs.pop_back();
      if (!devs.empty() && pIn && nIn) return memory_compress_lanes(pIn, nIn, pOut, nOutCap, nFlags, bs, pDict, nDictSize, devs);
   } catch (...) {   // (std::bad_alloc from the device list)
      return (size_t)-1;
   }
   // the whole input is at hand: size the device batch to it
   if (stream_init_sized(&strm, nFlags, nMaxBlockSize, nblocks ? nblocks : 1) != ZULTRA_OK) return (size_t)-1;
   if (pDict && nDictSize > 0 && zultra_stream_set_dictionary(&strm, pDict, nDictSize) != ZULTRA_OK) {
      zultra_stream_end(&strm);
      return (size_t)-1;
   }
   strm.next_in = pIn;
   strm.avail_in = nIn;
   strm.next_out = pOut;
   strm.avail_out = nOutCap;
   zultra_status_t st = zultra_stream_compress(&strm, ZULTRA_FINALIZE);
   zultra_stream_end(&strm);
   if (st != ZULTRA_STREAM_END) return (size_t)-1;
   return nOutCap - strm.avail_out;
}

extern "C" size_t zultra_memory_compress(const unsigned char *pIn, size_t nIn, unsigned char *pOut, size_t nOutCap,
                                         const unsigned int nFlags, unsigned int nMaxBlockSize) {
   return zultra_memory_compress_dict(pIn, nIn, pOut, nOutCap, nFlags, nMaxBlockSize, NULL, 0);
}

// ---- framed members: every max-block of a batch a complete gzip / zlib / BGZF member, written on the device ------------------------------
// (include/zultra_hip.h: zultra_hip_frame_members). One batch: compress, frame, verify if asked, one read of the framed bytes to `out`.
// data_mode as zultra_hip_compress_blocks' data_on_device. Returns the bytes written, (size_t)-1 on any failure (cap too small among them).
static size_t members_batch(zultra_hip_ctx_t *c, const uint8_t *data, size_t data_size, int data_mode, const zultra_hip_block_t *blocks, uint32_t count, unsigned framing,
                            int eof, uint8_t *out, size_t cap, zultra_hip_member_t *members) {
   uint64_t total = 0;
   if (zultra_hip_compress_blocks(c, data, data_size, data_mode, blocks, count) <= 0) return (size_t)-1;
   if (zultra_hip_frame_members(c, framing, eof, members, &total) != 0) return (size_t)-1;
   if (zh_verify_on() && !zh_verify_stitched(c)) return (size_t)-1;
   if (total > cap || zultra_hip_stream_read(c, out, 0, (size_t)total) != 0) return (size_t)-1;
   return (size_t)total;
}

static const unsigned char g_bgzf_eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// per member: header and trailer, and what zultra_memory_bound allows a max-block's stream beyond its input (64 sub-blocks, stored at worst)
extern "C" size_t zultra_memory_bound_bgzf(size_t nIn, unsigned int nBlockSize) {
   const size_t bs = nBlockSize ? nBlockSize : ZULTRA_HIP_BGZF_BLOCK;
   return nIn + ((nIn + bs - 1) / bs) * (18 + 8 + (1 + 4 + 1) * 64) + sizeof(g_bgzf_eof);
}

extern "C" size_t zultra_memory_compress_bgzf(const unsigned char *pIn, size_t nIn, unsigned char *pOut, size_t nMaxOut, unsigned int nBlockSize) try {
   // (a context of max-blocks of at most ZULTRA_HIP_BGZF_BLOCK bytes cannot produce an oversize member: include/zultra_hip.h)
   const uint32_t bs = nBlockSize ? nBlockSize : ZULTRA_HIP_BGZF_BLOCK;
   if (!pOut || (nIn && !pIn) || bs > ZULTRA_HIP_BGZF_BLOCK || zultra_hip_device_count() <= 0) return (size_t)-1;
   if (!nIn) {
      if (nMaxOut < sizeof(g_bgzf_eof)) return (size_t)-1;
      memcpy(pOut, g_bgzf_eof, sizeof(g_bgzf_eof));
      return sizeof(g_bgzf_eof);
   }
   const int dev = zh_pick_device();
   const uint32_t ctx_bs = zh_clamp_block(bs);
   const size_t total_blocks = (nIn + bs - 1) / bs;
   const uint32_t per = ctx_blocks(dev, ctx_bs, total_blocks);
   zultra_hip_ctx_t *c = ctx_acquire_on(dev, ctx_bs, per);
   if (!c) return (size_t)-1;
   std::vector<zultra_hip_block_t> blocks(per);
   std::vector<zultra_hip_member_t> members(per);
   size_t w = 0;
   for (size_t b = 0; b < total_blocks && w != (size_t)-1; b += per) {
      const size_t nb = total_blocks - b < per ? total_blocks - b : per, first = b * bs, bytes = nb * bs < nIn - first ? nb * bs : nIn - first;
      for (size_t k = 0; k < nb; k++) blocks[k] = zultra_hip_block_t{(uint64_t)k * bs, 0, (uint32_t)(k + 1 == nb ? bytes - k * bs : bs)};
      const size_t got = members_batch(c, pIn + first, bytes, 2, blocks.data(), (uint32_t)nb, ZULTRA_HIP_FRAME_BGZF, b + nb == total_blocks, pOut + w, nMaxOut - w, members.data());
      w = got == (size_t)-1 ? got : w + got;
   }
   ctx_release(c);
   return w;
} catch (...) {
   return (size_t)-1;
}

// The batches of n independent inputs, under zultra_memory_compress_batch and zultra_memory_compress_zip. Consecutive inputs of one kind — below 8192 bytes: a
// files context; from there on: a context of max-blocks as large as the call's largest input — share a batch, as many as the context takes; a batch's inputs are
// gathered into the context's pinned staging, max-block k at blocks[k].win_off, and per_batch(context, staging, bytes, blocks, i, j) does the rest for the inputs
// i .. j - 1. An input of size 0 is refused unless allow_empty; then it is no max-block and rides with the batch it sits in or next to (behind, where there is
// one): per_batch finds it by its size. A call of empty inputs only has no batch. Returns false where anything fails.
template <typename F>
static bool for_input_batches(const unsigned char *pIn, size_t nIn, const size_t *pInOff, const size_t *pInSize, size_t n, bool allow_empty, F per_batch) {
   const size_t small_limit = 8192;
   size_t largest = 0, nsmall = 0, nempty = 0;
   for (size_t i = 0; i < n; i++) {
      if (!pInSize[i] && allow_empty) {
         nempty++;
         continue;
      }
      if (!pInSize[i] || pInSize[i] > nIn || pInOff[i] > nIn - pInSize[i] || pInSize[i] > 2097152) return false;   // (an empty input is refused, as by zultra_memory_compress; a member is ONE max-block)
      largest = pInSize[i] > largest ? pInSize[i] : largest;
      nsmall += pInSize[i] < small_limit;
   }
   if (nempty == n) return true;
   const size_t nlarge = n - nempty - nsmall;
   const int dev = zh_pick_device();
   struct Ctxs {   // (the files context is this call's own: the cache keeps contexts of max-blocks)
      zultra_hip_ctx_t *files = NULL, *blocks = NULL;
      ~Ctxs() {
         if (files) zultra_hip_destroy(files);
         ctx_release(blocks);
      }
   } C;
   uint32_t files_cap = (uint32_t)(nsmall < 65536 ? nsmall : 65536);
   const uint32_t ctx_bs = zh_clamp_block((uint32_t)largest), blocks_cap = nlarge ? ctx_blocks(dev, ctx_bs, nlarge) : 0;
   // (a files context for fewer inputs per batch where the device has no room for the large one: down to 256, which is 10 MB or so)
   while (nsmall && !(C.files = zultra_hip_create_files(dev, (uint32_t)small_limit - 1, files_cap))) {
      if (files_cap <= 256) return false;
      files_cap = files_cap / 4 < 256 ? 256 : files_cap / 4;
   }
   if (nlarge && !(C.blocks = ctx_acquire_on(dev, ctx_bs, blocks_cap))) return false;
   std::vector<zultra_hip_block_t> blocks;
   for (size_t i = 0; i < n;) {
      size_t first = i;
      while (!pInSize[first]) first++;   // (there is one: empty inputs at the end went with the batch in front of them)
      const bool small = pInSize[first] < small_limit;
      zultra_hip_ctx_t *c = small ? C.files : C.blocks;
      const size_t max_count = small ? files_cap : blocks_cap, max_bytes = zultra_hip_data_capacity(c);
      size_t j = i, bytes = 0;
      blocks.clear();
      for (; j < n; j++) {
         if (!pInSize[j]) continue;
         if ((pInSize[j] < small_limit) != small || blocks.size() >= max_count || bytes + pInSize[j] > max_bytes) break;
         blocks.push_back(zultra_hip_block_t{(uint64_t)bytes, 0, (uint32_t)pInSize[j]});
         bytes += pInSize[j];
      }
      if (blocks.empty()) return false;
      uint8_t *stage = (uint8_t *)zultra_hip_staging(c, 0, bytes);
      if (!stage) return false;
      for (size_t k = i, b = 0; k < j; k++)
         if (pInSize[k]) memcpy(stage + blocks[b++].win_off, pIn + pInOff[k], pInSize[k]);
      if (!per_batch(c, stage, bytes, blocks, i, j)) return false;
      i = j;
   }
   return true;
}

extern "C" size_t zultra_memory_compress_batch(const unsigned char *pIn, size_t nIn, const size_t *pInOff, const size_t *pInSize, size_t n, unsigned char *pOut, size_t nMaxOut,
                                               size_t *pOutOff, const unsigned int nFlags) try {
   if (!pIn || !pInOff || !pInSize || !n || !pOut || !pOutOff || (nFlags != 0 && nFlags != ZULTRA_FLAG_ZLIB_FRAMING && nFlags != ZULTRA_FLAG_GZIP_FRAMING) || zultra_hip_device_count() <= 0)
      return (size_t)-1;
   std::vector<zultra_hip_member_t> members;
   size_t w = 0;
   // a batch's members are read to where they belong in pOut
   const bool ok = for_input_batches(pIn, nIn, pInOff, pInSize, n, false, [&](zultra_hip_ctx_t *c, const uint8_t *stage, size_t bytes, const std::vector<zultra_hip_block_t> &blocks, size_t i, size_t j) {
      members.resize(j - i);
      const size_t got = members_batch(c, stage, bytes, 0, blocks.data(), (uint32_t)(j - i), nFlags, 0, pOut + w, nMaxOut - w, members.data());
      if (got == (size_t)-1) return false;
      for (size_t k = i; k < j; k++) pOutOff[k] = w + (size_t)members[k - i].off;
      w += got;
      return true;
   });
   if (!ok) return (size_t)-1;
   pOutOff[n] = w;
   return w;
} catch (...) {
   return (size_t)-1;
}

// ---- ZIP archives: local records and the central directory written on the device (include/zultra_hip.h: zultra_hip_zip_members) -------------------------
static void zip_put(unsigned char *&p, unsigned long long v, int nbytes) {
   for (int k = 0; k < nbytes; k++) *p++ = (unsigned char)(v >> (8 * k));
}

extern "C" size_t zultra_zip_end_records(unsigned char *pOut, size_t nMaxOut, unsigned long long nEntries, unsigned long long nCentralOff, unsigned long long nCentralSize) {
   const bool zip64 = nEntries > 65535;
   if (!pOut || nMaxOut < (zip64 ? 98u : 22u) || nCentralOff >= 0xFFFFFFFFull || nCentralSize >= 0xFFFFFFFFull) return (size_t)-1;
   unsigned char *p = pOut;
   if (zip64) {
      zip_put(p, 0x06064b50, 4);   // the ZIP64 end record: size of what follows, version made by, version needed, disks, entries twice, the central directory
      zip_put(p, 44, 8);
      zip_put(p, 45, 2);
      zip_put(p, 45, 2);
      zip_put(p, 0, 4);
      zip_put(p, 0, 4);
      zip_put(p, nEntries, 8);
      zip_put(p, nEntries, 8);
      zip_put(p, nCentralSize, 8);
      zip_put(p, nCentralOff, 8);
      zip_put(p, 0x07064b50, 4);   // its locator: disk, where the record stands, disks in all
      zip_put(p, 0, 4);
      zip_put(p, nCentralOff + nCentralSize, 8);
      zip_put(p, 1, 4);
   }
   zip_put(p, 0x06054b50, 4);
   zip_put(p, 0, 2);
   zip_put(p, 0, 2);
   zip_put(p, zip64 ? 0xFFFF : nEntries, 2);
   zip_put(p, zip64 ? 0xFFFF : nEntries, 2);
   zip_put(p, nCentralSize, 4);
   zip_put(p, nCentralOff, 4);
   zip_put(p, 0, 2);
   return (size_t)(p - pOut);
}

// per entry: the two headers, and what zultra_memory_bound allows a max-block's stream beyond its input (64 sub-blocks, stored at worst); both copies of the names
extern "C" size_t zultra_memory_bound_zip(size_t nInTotal, size_t nNamesTotal, size_t n) { return nInTotal + 2 * nNamesTotal + n * (30 + 46 + (1 + 4 + 1) * 64 + 8) + 98; }

// The records of an archive of empty entries only, which has no batch for the device to hang them on: the layout of zh_zip_records for an empty entry.
static void zip_empty_entry(unsigned char *&p, bool central, const char *name, size_t name_len, unsigned int dos, unsigned long long local_off) {
   zip_put(p, central ? 0x02014b50 : 0x04034b50, 4);
   if (central) zip_put(p, 20, 2);
   zip_put(p, 10, 2);
   zip_put(p, 0x0800, 2);
   zip_put(p, 0, 2);
   zip_put(p, dos, 4);
   for (int k = 0; k < 3; k++) zip_put(p, 0, 4);   // CRC-32, sizes
   zip_put(p, name_len, 2);
   zip_put(p, 0, 2);
   if (central) {
      zip_put(p, 0, 6);   // comment, disk, internal attributes
      zip_put(p, 0, 4);   // external attributes
      zip_put(p, local_off, 4);
   }
   memcpy(p, name, name_len);
   p += name_len;
}

extern "C" size_t zultra_memory_compress_zip(const unsigned char *pIn, size_t nIn, const size_t *pInOff, const size_t *pInSize, const char *pNames, const size_t *pNameOff, size_t n,
                                             unsigned char *pOut, size_t nMaxOut, unsigned int nDosDateTime) try {
   if (!pInOff || !pInSize || !pNames || !pNameOff || !n || !pOut) return (size_t)-1;
   size_t nempty = 0;
   for (size_t i = 0; i < n; i++) {
      if (pNameOff[i + 1] <= pNameOff[i] || pNameOff[i + 1] - pNameOff[i] > 65535) return (size_t)-1;
      nempty += !pInSize[i];
   }
   const size_t names_total = pNameOff[n] - pNameOff[0];
   if (names_total >= 0xFFFFFFFFull || (nempty < n && (!pIn || zultra_hip_device_count() <= 0))) return (size_t)-1;
   const unsigned int dos = nDosDateTime ? nDosDateTime : 0x00210000u;
   std::vector<unsigned char> central;
   size_t w = 0;
   if (nempty == n) {
      if ((30 + 46) * n + 2 * names_total + 98 > nMaxOut || 30 * n + names_total >= 0xFFFFFFFFull) return (size_t)-1;
      central.resize(46 * n + names_total);
      unsigned char *l = pOut, *c = central.data();
      for (size_t i = 0; i < n; i++) {
         zip_empty_entry(c, true, pNames + pNameOff[i], pNameOff[i + 1] - pNameOff[i], dos, (unsigned long long)(l - pOut));
         zip_empty_entry(l, false, pNames + pNameOff[i], pNameOff[i + 1] - pNameOff[i], dos, 0);
      }
      w = (size_t)(l - pOut);
   }
   std::vector<uint32_t> name_off, entry_block;
   std::vector<uint64_t> file_off;
   const bool ok = for_input_batches(pIn, nIn, pInOff, pInSize, n, true, [&](zultra_hip_ctx_t *c, const uint8_t *stage, size_t bytes, const std::vector<zultra_hip_block_t> &blocks, size_t i, size_t j) {
      if (zultra_hip_compress_blocks(c, stage, bytes, 0, blocks.data(), (uint32_t)blocks.size()) <= 0) return false;
      if (zh_verify_on()) {   // (on the plain layout, which the gather leaves alone)
         file_off.resize(blocks.size() + 1);
         if (zultra_hip_stitch_files(c, file_off.data()) != 0 || !zh_verify_stitched(c)) return false;
      }
      name_off.resize(j - i + 1);
      entry_block.resize(j - i);
      for (size_t k = i; k <= j; k++) name_off[k - i] = (uint32_t)(pNameOff[k] - pNameOff[i]);
      for (size_t k = i, b = 0; k < j; k++) entry_block[k - i] = pInSize[k] ? (uint32_t)b++ : 0xFFFFFFFFu;
      uint64_t local = 0, cent = 0, central_at = 0;
      if (zultra_hip_zip_members(c, pNames + pNameOff[i], name_off.data(), entry_block.data(), (uint32_t)(j - i), w, dos, NULL, &local, &cent) != 0) return false;
      if (local > nMaxOut - w || zultra_hip_zip_read(c, pOut + w, 0, (size_t)local) != 0) return false;
      (void)zultra_hip_zip_device(c, &central_at);
      central.resize(central.size() + (size_t)cent);
      if (zultra_hip_zip_read(c, central.data() + central.size() - (size_t)cent, (size_t)central_at, (size_t)cent) != 0) return false;
      w += (size_t)local;
      return true;
   });
   if (!ok || central.size() > nMaxOut - w) return (size_t)-1;
   memcpy(pOut + w, central.data(), central.size());
   const size_t end = zultra_zip_end_records(pOut + w + central.size(), nMaxOut - w - central.size(), n, w, central.size());
   return end == (size_t)-1 ? end : w + central.size() + end;
} catch (...) {
   return (size_t)-1;
}

// ---- inputs of any size as streams of several max-blocks in one batch (include/zultra_hip.h: the grouped assembly) -----------------------------------
// The batches of n inputs, each a run of max-blocks of bs bytes with real history (batch_describe), under zultra_memory_compress_streams and
// zultra_memory_compress_zip_streams. An input lies wholly in one batch; a batch takes inputs while the context has max-blocks left. The inputs are gathered into
// the context's pinned staging one behind the other, and per_batch(context, stage, bytes, blocks, stream_first, i, j) does the rest for the inputs i .. j - 1 —
// stream_first has one entry per non-empty input of them. Empty inputs as in for_input_batches. Returns false where anything fails, an input with more
// max-blocks than the context holds among it.
template <typename F>
static bool for_stream_batches(const unsigned char *pIn, size_t nIn, const size_t *pInOff, const size_t *pInSize, size_t n, uint32_t bs, bool allow_empty, F per_batch) {
   uint64_t total_blocks = 0, most = 0;
   for (size_t i = 0; i < n; i++) {
      if (!pInSize[i] && allow_empty) continue;
      if (!pInSize[i] || pInSize[i] > nIn || pInOff[i] > nIn - pInSize[i] || pInSize[i] >= 0xFFFFFFFFull) return false;
      const uint64_t nb = ((uint64_t)pInSize[i] + bs - 1) / bs;
      total_blocks += nb;
      most = nb > most ? nb : most;
   }
   if (!total_blocks) return true;
   const int dev = zh_pick_device();
   const uint32_t cap = ctx_blocks(dev, bs, total_blocks);
   if (most > cap) return false;   // (one huge input is zultra_memory_compress's business)
   zultra_hip_ctx_t *c = ctx_acquire_on(dev, bs, cap);
   if (!c) return false;
   std::vector<zultra_hip_block_t> blocks;
   std::vector<uint32_t> stream_first;
   bool ok = true;
   for (size_t i = 0; ok && i < n;) {
      size_t j = i, bytes = 0;
      blocks.clear();
      stream_first.clear();
      for (; j < n; j++) {
         if (!pInSize[j]) continue;
         const size_t nb = (pInSize[j] + bs - 1) / bs;
         if (blocks.size() + nb > cap) break;
         stream_first.push_back((uint32_t)blocks.size());
         blocks.resize(blocks.size() + nb);
         zultra_hip_block_t *first = blocks.data() + stream_first.back();
         batch_describe(first, 0, bs, nb, (uint32_t)(pInSize[j] - (nb - 1) * bs));
         for (size_t k = 0; k < nb; k++) first[k].win_off += bytes;
         bytes += pInSize[j];
      }
      uint8_t *stage = blocks.empty() ? NULL : (uint8_t *)zultra_hip_staging(c, 0, bytes);
      if (!stage) {
         ok = false;
         break;
      }
      for (size_t k = i, s = 0; k < j; k++)
         if (pInSize[k]) zh_threaded_copy(stage + blocks[stream_first[s++]].win_off, pIn + pInOff[k], pInSize[k], 8u << 20);
      ok = per_batch(c, stage, bytes, blocks, stream_first, i, j);
      i = j;
   }
   ctx_release(c);
   return ok;
}

extern "C" size_t zultra_memory_compress_streams(const unsigned char *pIn, size_t nIn, const size_t *pInOff, const size_t *pInSize, size_t n, unsigned char *pOut, size_t nMaxOut,
                                                 size_t *pOutOff, const unsigned int nFlags, unsigned int nMaxBlockSize) try {
   if (!pIn || !pInOff || !pInSize || !n || !pOut || !pOutOff || (nFlags != 0 && nFlags != ZULTRA_FLAG_ZLIB_FRAMING && nFlags != ZULTRA_FLAG_GZIP_FRAMING) || zultra_hip_device_count() <= 0)
      return (size_t)-1;
   std::vector<zultra_hip_member_t> members;
   size_t w = 0;
   const bool ok = for_stream_batches(pIn, nIn, pInOff, pInSize, n, zh_clamp_block(nMaxBlockSize), false,
                                      [&](zultra_hip_ctx_t *c, const uint8_t *stage, size_t bytes, const std::vector<zultra_hip_block_t> &blocks, const std::vector<uint32_t> &stream_first, size_t i, size_t j) {
      uint64_t total = 0;
      members.resize(j - i);
      if (zultra_hip_compress_blocks(c, stage, bytes, 0, blocks.data(), (uint32_t)blocks.size()) <= 0) return false;
      if (zultra_hip_frame_streams(c, stream_first.data(), (uint32_t)stream_first.size(), nFlags, members.data(), &total) != 0) return false;
      if (zh_verify_on() && !zh_verify_stitched(c)) return false;
      if (total > nMaxOut - w || zultra_hip_stream_read(c, pOut + w, 0, (size_t)total) != 0) return false;
      for (size_t k = i; k < j; k++) pOutOff[k] = w + (size_t)members[k - i].off;
      w += (size_t)total;
      return true;
   });
   if (!ok) return (size_t)-1;
   pOutOff[n] = w;
   return w;
} catch (...) {
   return (size_t)-1;
}

extern "C" size_t zultra_memory_compress_zip_streams(const unsigned char *pIn, size_t nIn, const size_t *pInOff, const size_t *pInSize, const char *pNames, const size_t *pNameOff, size_t n,
                                                     unsigned char *pOut, size_t nMaxOut, unsigned int nDosDateTime, unsigned int nMaxBlockSize) try {
   if (!pInOff || !pInSize || !pNames || !pNameOff || !n || !pOut) return (size_t)-1;
   size_t nempty = 0;
   for (size_t i = 0; i < n; i++) nempty += !pInSize[i];
   if (nempty == n) return zultra_memory_compress_zip(pIn, nIn, pInOff, pInSize, pNames, pNameOff, n, pOut, nMaxOut, nDosDateTime);   // (no batch: the records are the host's)
   for (size_t i = 0; i < n; i++)
      if (pNameOff[i + 1] <= pNameOff[i] || pNameOff[i + 1] - pNameOff[i] > 65535) return (size_t)-1;
   if (pNameOff[n] - pNameOff[0] >= 0xFFFFFFFFull || !pIn || zultra_hip_device_count() <= 0) return (size_t)-1;
   const unsigned int dos = nDosDateTime ? nDosDateTime : 0x00210000u;
   std::vector<unsigned char> central;
   std::vector<uint32_t> name_off, entry_stream;
   std::vector<zultra_hip_member_t> members;
   size_t w = 0;
   const bool ok = for_stream_batches(pIn, nIn, pInOff, pInSize, n, zh_clamp_block(nMaxBlockSize), true,
                                      [&](zultra_hip_ctx_t *c, const uint8_t *stage, size_t bytes, const std::vector<zultra_hip_block_t> &blocks, const std::vector<uint32_t> &stream_first, size_t i, size_t j) {
      const uint32_t nstreams = (uint32_t)stream_first.size();
      if (zultra_hip_compress_blocks(c, stage, bytes, 0, blocks.data(), (uint32_t)blocks.size()) <= 0) return false;
      if (zh_verify_on()) {   // (on the plain grouped layout, which the gather then finds in place)
         uint64_t total = 0;
         members.resize(nstreams);
         if (zultra_hip_frame_streams(c, stream_first.data(), nstreams, 0, members.data(), &total) != 0 || !zh_verify_stitched(c)) return false;
      }
      name_off.resize(j - i + 1);
      entry_stream.resize(j - i);
      for (size_t k = i; k <= j; k++) name_off[k - i] = (uint32_t)(pNameOff[k] - pNameOff[i]);
      for (size_t k = i, s = 0; k < j; k++) entry_stream[k - i] = pInSize[k] ? (uint32_t)s++ : 0xFFFFFFFFu;
      uint64_t local = 0, cent = 0, central_at = 0;
      if (zultra_hip_zip_streams(c, stream_first.data(), nstreams, pNames + pNameOff[i], name_off.data(), entry_stream.data(), (uint32_t)(j - i), w, dos, NULL, &local, &cent) != 0) return false;
      if (local > nMaxOut - w || zultra_hip_zip_read(c, pOut + w, 0, (size_t)local) != 0) return false;
      (void)zultra_hip_zip_device(c, &central_at);
      central.resize(central.size() + (size_t)cent);
      if (zultra_hip_zip_read(c, central.data() + central.size() - (size_t)cent, (size_t)central_at, (size_t)cent) != 0) return false;
      w += (size_t)local;
      return true;
   });
   if (!ok || central.size() > nMaxOut - w) return (size_t)-1;
   memcpy(pOut + w, central.data(), central.size());
   const size_t end = zultra_zip_end_records(pOut + w + central.size(), nMaxOut - w - central.size(), n, w, central.size());
   return end == (size_t)-1 ? end : w + central.size() + end;
} catch (...) {
   return (size_t)-1;
}

// ================================================================================================================
// Decompression: the framing on the host, the deflate stream on the device (zultra_hip_inflate_streams)
// ================================================================================================================

// with_dict: zultra_memory_decompress_dict (a zlib stream may carry FDICT, and pDict — NULL for none — is the history of the deflate stream)
static size_t memory_decompress(const unsigned char *pIn, size_t nIn, unsigned char *pOut, size_t nMaxOut, const unsigned int nFlags, bool with_dict, const void *pDict, int nDictSize) {
   if (!pIn || (!pOut && nMaxOut)) return (size_t)-1;
   if (!pDict || nDictSize <= 0) {
      pDict = NULL;
      nDictSize = 0;
   }
   size_t head = 0, foot = 0;
   if (nFlags & ZULTRA_FLAG_GZIP_FRAMING) {
      // RFC 1952 2.3: ID1 ID2 CM FLG MTIME(4) XFL OS, then what FLG announces
      if (nIn < 18 || pIn[0] != 0x1f || pIn[1] != 0x8b || pIn[2] != 8 || (pIn[3] & 0xe0)) return (size_t)-1;
      const unsigned flg = pIn[3];
      head = 10;
      if (flg & 4) {   // FEXTRA: XLEN, then XLEN bytes
         if (head + 2 > nIn) return (size_t)-1;
         head += 2 + ((size_t)pIn[head] | ((size_t)pIn[head + 1] << 8));
      }
      for (unsigned bit = 8; bit <= 16; bit <<= 1)   // FNAME, FCOMMENT: zero-terminated
         if (flg & bit) {
            while (head < nIn && pIn[head]) head++;
            head++;
         }
      if (flg & 2) head += 2;   // FHCRC
      foot = 8;
   }
   else if (nFlags & ZULTRA_FLAG_ZLIB_FRAMING) {
      // RFC 1950 2.2: CM = 8, CINFO <= 7, (CMF * 256 + FLG) % 31 == 0; FDICT only where a dictionary may be given
      if (nIn < 6 || (pIn[0] & 15) != 8 || (pIn[0] >> 4) > 7 || (((unsigned)pIn[0] << 8) | pIn[1]) % 31 || ((pIn[1] & 0x20) && !with_dict)) return (size_t)-1;
      head = 2;
      foot = 4;
      if (pIn[1] & 0x20) {
         // DICTID: the Adler-32 of the whole dictionary, of which the last 32768 bytes are the history (zultra_frame_encode_header writes the same)
         if (!pDict) return (size_t)-1;
         const uint32_t id = ((uint32_t)pIn[2] << 24) | (pIn[3] << 16) | (pIn[4] << 8) | pIn[5];
         if (id != adler32_update(1, (const uint8_t *)pDict, (size_t)nDictSize)) return (size_t)-1;
         head = 6;
      }
      else
         nDictSize = 0;   // (no FDICT: the dictionary is not looked at, as in zlib)
   }
   if (head > nIn || foot > nIn - head || nIn - head - foot == 0) return (size_t)-1;
   const size_t nBody = nIn - head - foot;
   zultra_hip_inflate_item_t item = {0, nBody, 0, nMaxOut};
   zultra_hip_inflate_result_t res;
   unsigned char none = 0;
   if ((nDictSize ? zultra_hip_inflate_streams_dict(zh_pick_device(), pIn + head, nBody, 0, pOut ? pOut : &none, nMaxOut, 0, pDict, (size_t)nDictSize, 0, &item, 1, &res, NULL)
                  : zultra_hip_inflate_streams(zh_pick_device(), pIn + head, nBody, 0, pOut ? pOut : &none, nMaxOut, 0, &item, 1, &res, NULL)) != 0)
      return (size_t)-1;
   if (res.src_used != nBody) return (size_t)-1;   // (bytes behind the final block)
   const size_t nOut = (size_t)res.out_size;
   if (foot) {
      const unsigned char *f = pIn + head + nBody;
      const zultra_frame_checksum_t sum = zultra_frame_update_checksum(zultra_frame_init_checksum(nFlags), pOut, nOut, nFlags);
      if (nFlags & ZULTRA_FLAG_GZIP_FRAMING) {
         const uint32_t crc = f[0] | (f[1] << 8) | (f[2] << 16) | ((uint32_t)f[3] << 24), isize = f[4] | (f[5] << 8) | (f[6] << 16) | ((uint32_t)f[7] << 24);
         if (crc != sum || isize != (uint32_t)nOut) return (size_t)-1;
      }
      else if ((((uint32_t)f[0] << 24) | (f[1] << 16) | (f[2] << 8) | f[3]) != sum)
         return (size_t)-1;
   }
   return nOut;
}

extern "C" size_t zultra_memory_decompress(const unsigned char *pIn, size_t nIn, unsigned char *pOut, size_t nMaxOut, const unsigned int nFlags) {
   return memory_decompress(pIn, nIn, pOut, nMaxOut, nFlags, false, NULL, 0);
}

extern "C" size_t zultra_memory_decompress_dict(const unsigned char *pIn, size_t nIn, unsigned char *pOut, size_t nMaxOut, const unsigned int nFlags, const void *pDict, int nDictSize) {
   return memory_decompress(pIn, nIn, pOut, nMaxOut, nFlags, true, pDict, nDictSize);
}

// Many members of one framing: all of it on the device (zultra_hip_inflate_members), from and to host memory
extern "C" size_t zultra_memory_decompress_batch(const unsigned char *pIn, size_t nIn, const size_t *pInOff, const size_t *pInSize, unsigned char *pOut, size_t nMaxOut,
                                                 const size_t *pOutOff, const size_t *pOutCap, size_t *pOutSize, size_t n, const unsigned int nFlags, const void *pDict, int nDictSize) {
   const unsigned int framing = nFlags & (ZULTRA_FLAG_ZLIB_FRAMING | ZULTRA_FLAG_GZIP_FRAMING);
   if (!pIn || (!pOut && nMaxOut) || !pInOff || !pInSize || !pOutOff || !pOutCap || !pOutSize || n == 0 || n > 0xFFFFFFFFull ||
       framing == (ZULTRA_FLAG_ZLIB_FRAMING | ZULTRA_FLAG_GZIP_FRAMING))
      return (size_t)-1;
   if (!pDict || nDictSize <= 0) {
      pDict = NULL;
      nDictSize = 0;
   }
   std::vector<zultra_hip_inflate_item_t> items(n);
   std::vector<zultra_hip_member_result_t> res(n);
   for (size_t i = 0; i < n; i++) items[i] = {pInOff[i], pInSize[i], pOutOff[i], pOutCap[i]};
   unsigned char none = 0;
   if (zultra_hip_inflate_members(zh_pick_device(), pIn, nIn, 0, pOut ? pOut : &none, nMaxOut, 0, pDict, (size_t)nDictSize, 0, framing, items.data(), (uint32_t)n, res.data(), NULL) < 0)
      return (size_t)-1;
   size_t failed = 0;
   for (size_t i = 0; i < n; i++) {
      const bool ok = res[i].reason == 0 && res[i].src_used == pInSize[i];   // (bytes behind the trailer)
      pOutSize[i] = ok ? (size_t)res[i].out_size : (size_t)-1;
      failed += !ok;
   }
   return failed;
}

// gzip(1) over a whole file: runs of hinted members through zultra_hip_inflate_file, a member without a hint through zultra_hip_inflate_members on its own
extern "C" size_t zultra_memory_decompress_members(const unsigned char *pIn, size_t nIn, unsigned char *pOut, size_t nMaxOut, size_t *pnMembers) {
   if (pnMembers) *pnMembers = 0;
   if (!pIn || nIn == 0 || (!pOut && nMaxOut)) return (size_t)-1;
   const int device = zh_pick_device();
   uint8_t *const d_in = (uint8_t *)zh_device_upload(device, pIn, nIn);
   if (!d_in) return (size_t)-1;
   unsigned char none = 0;
   size_t at = 0, written = 0, members = 0;
   bool ok = true;
   while (ok) {
      unsigned char *const out = pOut ? pOut + written : &none;
      zultra_hip_index_result_t ix;
      if (zultra_hip_inflate_file(device, d_in + at, nIn - at, 1, out, nMaxOut - written, 0, &ix, NULL, 0, NULL) != 0) ok = false;   // a member failed, too little room, an error
      else {
         at += (size_t)ix.src_used;
         written += (size_t)ix.out_size;
         members += ix.members;
         if (ix.stop == 0) break;
         if (ix.stop != 1) ok = false;   // cut off, garbage, zeros
         else {
            // a gzip member the index cannot size: the rest of the file is its item, the room left its room; src_used says where it ends
            const zultra_hip_inflate_item_t item = {0, nIn - at, 0, nMaxOut - written};
            zultra_hip_member_result_t r;
            if (zultra_hip_inflate_members(device, d_in + at, nIn - at, 1, pOut ? pOut + written : &none, nMaxOut - written, 0, NULL, 0, 0, ZULTRA_FLAG_GZIP_FRAMING, &item, 1, &r, NULL) != 0 || r.src_used == 0) ok = false;
            else {
               at += (size_t)r.src_used;
               written += (size_t)r.out_size;
               members++;
               if (at == nIn) break;
            }
         }
      }
   }
   zh_device_release(d_in);
   if (!ok) return (size_t)-1;
   if (pnMembers) *pnMembers = members;
   return written;
}

// ---- a byte range of a BGZF file, and bgzip's .gzi index (include/zultra_hip.h: zultra_hip_inflate_range) ----------------------------------------------
static unsigned long long gzi_get(const unsigned char *p) {
   unsigned long long v = 0;
   for (int k = 0; k < 8; k++) v |= (unsigned long long)p[k] << (8 * k);
   return v;
}
static void gzi_put(unsigned char *p, unsigned long long v) {
   for (int k = 0; k < 8; k++) p[k] = (unsigned char)(v >> (8 * k));
}

// One pair for every indexed member but the first. The source is uploaded once: the index runs over it twice, for the count and for the items.
extern "C" size_t zultra_memory_index_gzi(const unsigned char *pIn, size_t nIn, unsigned char *pGzi, size_t nMaxGzi) try {
   if (!pIn || nIn == 0) return (size_t)-1;
   const int device = zh_pick_device();
   uint8_t *const d_in = (uint8_t *)zh_device_upload(device, pIn, nIn);
   if (!d_in) return (size_t)-1;
   size_t size = (size_t)-1;
   zultra_hip_index_result_t ix;
   if (zultra_hip_index_members(device, d_in, nIn, 1, NULL, 0, &ix, NULL) == 0 && ix.stop == 0 && ix.members >= 1) {
      const size_t n = ix.members - 1;
      size = 8 + 16 * n;
      if (pGzi && nMaxGzi < size) size = (size_t)-1;
      else if (pGzi) {
         std::vector<zultra_hip_inflate_item_t> items(ix.members);
         if (zultra_hip_index_members(device, d_in, nIn, 1, items.data(), ix.members, &ix, NULL) != 0 || ix.stop != 0 || ix.members != n + 1) size = (size_t)-1;
         else {
            gzi_put(pGzi, n);
            for (size_t i = 0; i < n; i++) {
               gzi_put(pGzi + 8 + 16 * i, items[i + 1].src_off);
               gzi_put(pGzi + 16 + 16 * i, items[i + 1].dst_off);
            }
         }
      }
   }
   zh_device_release(d_in);
   return size;
}
catch (...) {
   return (size_t)-1;
}

extern "C" size_t zultra_memory_decompress_range(const unsigned char *pIn, size_t nIn, unsigned long long nFirst, size_t nBytes, unsigned char *pOut, size_t nMaxOut,
                                                 const unsigned char *pGzi, size_t nGzi) {
   if (!pIn || nIn == 0 || (!pOut && nMaxOut) || (!pGzi && nGzi)) return (size_t)-1;
   const int device = zh_pick_device();
   unsigned char none = 0;
   unsigned char *const out = pOut ? pOut : &none;
   const unsigned long long end = (unsigned long long)nBytes > ~0ull - nFirst ? ~0ull : nFirst + nBytes;
   zultra_hip_range_result_t res;
   if (!pGzi) {
      if (zultra_hip_inflate_range(device, pIn, nIn, 0, nFirst, nBytes, out, nMaxOut, 0, &res, NULL, 0, NULL) != 0) return (size_t)-1;   // a member failed, too little room, an error
      if (res.stop != 0 && end > res.file_size) return (size_t)-1;   // what lies behind the indexed prefix is unknown
      return (size_t)res.out_size;
   }
   // the index: well-formed, and in order
   if (nGzi < 8 || (nGzi - 8) % 16 != 0 || gzi_get(pGzi) != (nGzi - 8) / 16) return (size_t)-1;
   const size_t n = (nGzi - 8) / 16;
   const auto coff = [pGzi](size_t i) { return gzi_get(pGzi + 8 + 16 * i); };
   const auto uoff = [pGzi](size_t i) { return gzi_get(pGzi + 16 + 16 * i); };
   for (size_t i = 0; i < n; i++)
      if (coff(i) == 0 || coff(i) >= nIn || (i && (coff(i) <= coff(i - 1) || uoff(i) < uoff(i - 1)))) return (size_t)-1;
   if (nBytes == 0) return 0;
   // (c0, u0): the last pair with u <= nFirst; (c1, u1): the first with u >= end (behind the former, as end > nFirst)
   size_t lo = 0, hi = n;   // pairs [0, lo) have u <= nFirst
   while (lo < hi) {
      const size_t mid = lo + (hi - lo) / 2;
      if (uoff(mid) <= nFirst) lo = mid + 1;
      else hi = mid;
   }
   const unsigned long long c0 = lo ? coff(lo - 1) : 0, u0 = lo ? uoff(lo - 1) : 0;
   size_t at = lo;
   hi = n;   // pairs [lo, at) have u < end
   while (at < hi) {
      const size_t mid = at + (hi - at) / 2;
      if (uoff(mid) < end) at = mid + 1;
      else hi = mid;
   }
   const bool bounded = at < n;
   const unsigned long long c1 = bounded ? coff(at) : nIn, u1 = bounded ? uoff(at) : 0;
   if (zultra_hip_inflate_range(device, pIn + c0, (size_t)(c1 - c0), 0, nFirst - u0, nBytes, out, nMaxOut, 0, &res, NULL, 0, NULL) != 0) return (size_t)-1;
   // what the index said of the window: a member at its first byte, the chain's end at its last, and the output between the two pairs
   if (res.members == 0 || res.stop != 0 || (bounded && res.file_size != u1 - u0)) return (size_t)-1;
   return (size_t)res.out_size;
}

// ---- ZIP archives read: the end records on the host, everything else on the device (include/zultra_hip.h: zultra_hip_unzip) ---------------------------
static unsigned long long zip_get(const unsigned char *p, int nbytes) {
   unsigned long long v = 0;
   for (int k = 0; k < nbytes; k++) v |= (unsigned long long)p[k] << (8 * k);
   return v;
}

extern "C" int zultra_zip_find_end(const unsigned char *pTail, size_t nTail, unsigned long long nArchiveSize, zultra_zip_end_t *pEnd) {
   if (!pTail || !pEnd || nTail < 22 || nTail > nArchiveSize) return -1;
   const unsigned long long tail_at = nArchiveSize - nTail;   // the tail's position in the archive
   size_t p = nTail - 22;
   for (;; p--) {   // the last end record whose comment reaches the archive's end exactly
      if (zip_get(pTail + p, 4) == 0x06054b50 && p + 22 + zip_get(pTail + p + 20, 2) == nTail) break;
      if (p == 0) return -1;
   }
   if (zip_get(pTail + p + 4, 2) != 0 || zip_get(pTail + p + 6, 2) != 0) return -1;   // this disk, the directory's disk
   zultra_zip_end_t e;
   e.nEntries = zip_get(pTail + p + 10, 2);
   e.nCentralSize = zip_get(pTail + p + 12, 4);
   e.nCentralOff = zip_get(pTail + p + 16, 4);
   e.nZip64 = 0;
   unsigned long long dir_end = tail_at + p;
   if (p >= 20 && zip_get(pTail + p - 20, 4) == 0x07064b50) {
      const unsigned char *loc = pTail + p - 20;
      if (zip_get(loc + 4, 4) != 0 || zip_get(loc + 16, 4) != 1) return -1;
      // the record: where the locator says, or — behind a prefix the locator does not count — directly in front of the locator
      const unsigned long long named = zip_get(loc + 8, 8);
      size_t at = (size_t)-1;
      if (named >= tail_at && named - tail_at <= p - 20 && p - 20 - (size_t)(named - tail_at) >= 56 && zip_get(pTail + (size_t)(named - tail_at), 4) == 0x06064b50)
         at = (size_t)(named - tail_at);
      else if (p - 20 >= 56 && zip_get(pTail + p - 76, 4) == 0x06064b50)
         at = p - 76;
      if (at == (size_t)-1) return -1;
      const unsigned char *r = pTail + at;
      if (zip_get(r + 16, 4) != 0 || zip_get(r + 20, 4) != 0) return -1;
      e.nEntries = zip_get(r + 32, 8);
      e.nCentralSize = zip_get(r + 40, 8);
      e.nCentralOff = zip_get(r + 48, 8);
      e.nZip64 = 1;
      dir_end = tail_at + at;
   }
   else if (e.nCentralSize == 0xFFFFFFFFull || e.nCentralOff == 0xFFFFFFFFull)
      return -1;
   if (e.nCentralSize > dir_end || e.nCentralOff > dir_end - e.nCentralSize) return -1;   // a negative prefix
   e.nPrefix = dir_end - e.nCentralSize - e.nCentralOff;
   *pEnd = e;
   return 0;
}

extern "C" size_t zultra_memory_decompress_zip(const unsigned char *pIn, size_t nIn, unsigned char *pOut, size_t nMaxOut, zultra_zip_info_t *pInfo, size_t nMaxInfo, size_t *pnEntries) {
   if (pnEntries) *pnEntries = 0;
   if (!pIn || nIn == 0 || (!pOut && nMaxOut) || (!pInfo && nMaxInfo)) return (size_t)-1;
   const size_t tail = nIn < 65535 + 22 + 20 + 56 ? nIn : 65535 + 22 + 20 + 56;
   zultra_zip_end_t end;
   if (zultra_zip_find_end(pIn + nIn - tail, tail, nIn, &end) != 0) return (size_t)-1;
   const unsigned long long central_at = end.nPrefix + end.nCentralOff;
   if (end.nCentralSize / 46 < end.nEntries) return (size_t)-1;   // (more entries than the directory has room for: nothing is allocated for such a count)
   const int device = zh_pick_device();
   uint8_t *const d_in = (uint8_t *)zh_device_upload(device, pIn, nIn);
   if (!d_in) return (size_t)-1;
   const uint32_t cap = (uint32_t)zh_min64(end.nEntries, 0xFFFFFFFFull);
   std::vector<zultra_hip_zip_dirent_t> dirents(cap ? cap : 1);
   std::vector<zultra_hip_member_result_t> results(cap ? cap : 1);   // (zero-initialised: list-only leaves every status 0)
   zultra_hip_zip_index_result_t res = {};
   const bool list = pOut == NULL;
   int rc;
   if (list)
      rc = zultra_hip_zip_index(device, d_in, nIn, 1, central_at, end.nCentralSize, cap ? dirents.data() : NULL, cap, &res, NULL);
   else
      rc = zultra_hip_unzip(device, d_in, nIn, 1, central_at, end.nCentralSize, (int64_t)end.nPrefix, pOut, nMaxOut, 0, &res, dirents.data(), results.data(), cap ? cap : 1, NULL);
   // more output than nMaxOut (stop 4 with the end record's count): nothing was written and the directory was not read back; the infos are known all the
   // same, from the index alone. That runs the index kernels a second time, over the copy of the archive that is in device memory already: the price of an
   // error path, paid so that zultra_hip_unzip's refusal stays one that writes nothing
   const bool again = rc < 0 && !list && res.stop == 4 && res.entries == cap && cap != 0;
   const int irc = again ? zultra_hip_zip_index(device, d_in, nIn, 1, central_at, end.nCentralSize, dirents.data(), cap, &res, NULL) : 0;
   zh_device_release(d_in);
   if ((rc < 0 && !again) || irc != 0) {
      if (pnEntries && res.stop == 4) *pnEntries = res.entries;
      return (size_t)-1;
   }
   if (pnEntries) *pnEntries = res.entries;
   bool ok = rc >= 0 && res.stop == 0 && res.entries == end.nEntries && res.entries <= nMaxInfo;
   for (uint32_t i = 0; i < res.entries; i++) {
      const zultra_hip_zip_dirent_t &d = dirents[i];
      const zultra_hip_member_result_t &r = results[i];
      if (r.reason != 0 || (!list && rc >= 0 && d.method == 8 && r.src_used != d.comp_size)) ok = false;   // (a deflated entry fills its range, as a member of zultra_memory_decompress_batch does)
      if (i < nMaxInfo) {
         zultra_zip_info_t &o = pInfo[i];
         o.nNameAt = d.central_at + 46;
         o.nNameLen = d.name_len;
         o.nMethod = d.method;
         o.nFlags = d.flags;
         o.nCrc32 = d.crc32;
         o.nCompSize = d.comp_size;
         o.nSize = d.size;
         o.nOutOff = d.dst_off;
         o.nStatus = r.reason;
      }
   }
   return ok ? (size_t)res.out_size : (size_t)-1;
}
