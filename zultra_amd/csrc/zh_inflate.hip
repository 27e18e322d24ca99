// zh_inflate.hip — host side of the context-free inflate calls of include/zultra_hip.h: batches of raw streams (with or without a preset dictionary), batches
// of gzip / zlib members, the member index of a whole file, the whole file, a byte range of it, a ZIP archive's directory and its entries. No zultra_hip_ctx_t: a call owns what it allocates and releases it when it returns.
#include <zh_platform.h>

#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/zultra_hip.h"
#include "zh_host.h"
#include "zh_inflate_out.h"
#include "zh_inflate_check.h"
#include "zh_inflate_index.h"
#include "zh_inflate_range.h"
#include "zh_unzip.h"

// ---- batched inflate (zh_inflate_out.h, zh_inflate_check.h) -------------------------------------------------------------------------------------------
static_assert(sizeof(zultra_hip_inflate_item_t) == sizeof(zh_inflate_item_t) && sizeof(zultra_hip_inflate_result_t) == sizeof(zh_inflate_result_t), "ABI");
static_assert(sizeof(zultra_hip_member_result_t) == sizeof(zh_member_result_t), "ABI");

// Events of a call, on the null stream: the boundaries between which its kernel times are taken. A call creates the range of them that it marks.
enum zh_inflate_event {
   ZH_IEV_INDEX_START, ZH_IEV_INDEX_END, ZH_IEV_ITEMS_START, ZH_IEV_ITEMS_END,   // around zh_ix_tiles and zh_ix_resolve; around zh_ix_items
   ZH_IEV_HEADS, ZH_IEV_INFLATE, ZH_IEV_CHECKS, ZH_IEV_END,   // starts of zh_frame_heads, of the inflate kernel (a streams call's first mark), of zh_check_members; the end
   ZH_IEV_RG_PLAN, ZH_IEV_RG_ITEMS, ZH_IEV_RG_END,   // zultra_hip_inflate_range: behind zh_rg_select (the items' START in front of it), in front of zh_rg_items (their END behind it), behind zh_rg_edges
   ZH_IEV_UZ_LOCALS, ZH_IEV_UZ_INFLATE, ZH_IEV_UZ_COPY, ZH_IEV_UZ_CHECKS, ZH_IEV_UZ_END,   // zultra_hip_unzip: starts of zh_uz_locals, the inflate kernel, zh_uz_copy, zh_check_members; the end
   ZH_INFLATE_EVENTS
};
// a one-item batch of zh_check_members whose "output" is a device dictionary (zh_dictid)
struct zh_dictjob_t {
   zh_inflate_item_t item;
   zh_inflate_result_t inner;
   zh_member_result_t member;
   uint32_t idx;
};

// what a call holds on the device: released when the call returns, however it returns
struct zh_inflate_call_t {
   uint8_t *d_src = NULL, *d_dst = NULL, *d_hist = NULL;   // the staging of host pointers
   zh_inflate_item_t *d_items = NULL, *d_inner = NULL;     // (d_inner and everything below but the index's: members only)
   zh_inflate_result_t *d_results = NULL;
   zh_member_result_t *d_members = NULL;
   uint32_t *d_idx = NULL, *d_tables = NULL;
   uint32_t nsmall = 0, nlarge = 0, spg = 1;   // (zh_check_plan: how idx splits between the checksum kernel's two forms)
   zh_dictjob_t *d_dictjob = NULL;
   zh_ix_tile_t *d_ix_tiles = NULL;   // (the member index only)
   zh_ix_totals_t *d_ix_totals = NULL;
   zh_rg_plan_t *d_plan = NULL;   // (a range only, as the next: the members that straddle an end of it, decoded in full)
   uint8_t *d_edge = NULL;
   zh_zip_dirent_t *d_dirents = NULL;   // (a ZIP archive only, as the two below)
   zh_uz_copy_t *d_copies = NULL;
   uint32_t *d_ncopies = NULL;
   hipEvent_t ev[ZH_INFLATE_EVENTS] = {};
   std::vector<uint32_t> order;   // the items with room, by dst_off
   const uint8_t *s8 = NULL, *hist = NULL;   // (hist: the last hist_len bytes of the call's dictionary, where the kernel reads them)
   uint8_t *d8 = NULL;
   uint32_t hist_len = 0;
   ~zh_inflate_call_t() {
      for (void *p : std::initializer_list<void *>{d_src, d_dst, d_hist, d_items, d_inner, d_results, d_members, d_idx, d_tables, d_dictjob, d_ix_tiles, d_ix_totals, d_plan, d_edge, d_dirents, d_copies, d_ncopies}) (void)hipFree(p);
      for (hipEvent_t e : ev)
         if (e) (void)hipEventDestroy(e);
   }
};
#define ZH_TRY(call)                       \
   do {                                    \
      if ((call) != hipSuccess) return -1; \
   } while (0)

template <typename T>
static hipError_t zh_dalloc(T **p, size_t count) { return hipMalloc((void **)p, count * sizeof(T)); }
// CUs of the device, 256 if it does not say
ZH_HIDDEN uint32_t zh_device_cus(int device) {
   int cus = 0;
   if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
   return (uint32_t)cus;
}
// ZULTRA_HIP_GRID_CAP (tests: fewer waves or workgroups than pieces of work, every one strides), 0 without
static uint32_t zh_grid_cap() { return (uint32_t)max(0, zh_env("ZULTRA_HIP_GRID_CAP", 0)); }
static uint32_t zh_capped(uint32_t grid, uint32_t cap) { return cap ? max(1u, min(grid, cap)) : grid; }

// The steps of a call, each 0 or -1. No context: the call owns its item and result buffers (and, for host pointers, the staging of the source, of the output
// and of the history in device memory), on the null stream of `device`.
// 1. the arguments: every item inside its buffer, no two destination ranges over the same byte (empty ranges take none), no device history inside one.
// Of a preset dictionary the last min(dict_size, 32768) bytes are the history (zlib's inflateSetDictionary keeps the same).
static int zh_inflate_args(zh_inflate_call_t &C, int device, const void *src, size_t src_size, void *dst, size_t dst_size, int dst_on_device, const void *dict, size_t dict_size,
                           int dict_on_device, const zultra_hip_inflate_item_t *items, uint32_t n, const void *results) {
   if (!src || !dst || !items || !results || n == 0 || device < 0 || (!dict && dict_size)) return -1;
   C.hist_len = (uint32_t)zh_min64(dict_size, ZH_MAX_DIST);
   C.hist = dict ? (const uint8_t *)dict + (dict_size - C.hist_len) : NULL;
   std::vector<uint32_t> &order = C.order;
   order.reserve(n);
   for (uint32_t k = 0; k < n; k++) {
      const zultra_hip_inflate_item_t &it = items[k];
      if (it.src_off > src_size || it.src_size > src_size - it.src_off || it.dst_off > dst_size || it.dst_cap > dst_size - it.dst_off) return -1;
      if (it.dst_cap) order.push_back(k);
   }
   std::sort(order.begin(), order.end(), [items](uint32_t a, uint32_t b) { return items[a].dst_off < items[b].dst_off; });
   for (size_t i = 1; i < order.size(); i++)
      if (items[order[i - 1]].dst_off + items[order[i - 1]].dst_cap > items[order[i]].dst_off) return -1;
   if (C.hist_len && dict_on_device && dst_on_device) {   // the history is read while the output is written: none of it inside a destination range
      const uintptr_t h_lo = (uintptr_t)C.hist, h_hi = h_lo + C.hist_len;
      for (uint32_t k : order) {
         const uintptr_t d_lo = (uintptr_t)dst + items[k].dst_off;
         if (d_lo < h_hi && h_lo < d_lo + items[k].dst_cap) return -1;
      }
   }
   if (device >= zultra_hip_device_count()) return -1;
   return 0;
}
// 2. the device, the call's buffers, the events `first` to `last`, the staging of host pointers, the items uploaded
static int zh_inflate_stage(zh_inflate_call_t &C, int device, const void *src, size_t src_size, int src_on_device, void *dst, size_t dst_size, int dst_on_device, int dict_on_device,
                            const zultra_hip_inflate_item_t *items, uint32_t n, int first, int last) {
   ZH_TRY(hipSetDevice(device));
   ZH_TRY(zh_dalloc(&C.d_items, n));
   ZH_TRY(zh_dalloc(&C.d_results, n));
   for (int e = first; e <= last; e++) ZH_TRY(hipEventCreate(&C.ev[e]));
   C.s8 = (const uint8_t *)src;
   C.d8 = (uint8_t *)dst;
   if (!src_on_device) {
      ZH_TRY(zh_dalloc(&C.d_src, src_size ? src_size : 1));
      ZH_TRY(hipMemcpy(C.d_src, src, src_size, hipMemcpyHostToDevice));
      C.s8 = C.d_src;
   }
   if (!dst_on_device) {
      ZH_TRY(zh_dalloc(&C.d_dst, dst_size ? dst_size : 1));
      C.d8 = C.d_dst;
   }
   if (C.hist_len && !dict_on_device) {
      ZH_TRY(zh_dalloc(&C.d_hist, C.hist_len));
      ZH_TRY(hipMemcpy(C.d_hist, C.hist, C.hist_len, hipMemcpyHostToDevice));
      C.hist = C.d_hist;
   }
   ZH_TRY(hipMemcpy(C.d_items, items, (size_t)n * sizeof(zh_inflate_item_t), hipMemcpyHostToDevice));
   return 0;
}
// 3. the inflate kernel over n items that lie in device memory. C.hist_len == 0: zh_inflate_streams; else the last hist_len bytes of the dictionary
// (C.hist, at most 32768) lie in front of every item's output, zh_inflate_streams_dict.
static int zh_inflate_launch(const zh_inflate_call_t &C, int device, size_t src_size, size_t dst_size, const zh_inflate_item_t *d_items, uint32_t n) {
   const uint32_t grid = zh_capped((uint32_t)zh_min64(n, zh_max64(32ull * zh_device_cus(device), 64)), zh_grid_cap());   // (one wave per workgroup; a CU holds fewer at a time — zh_inflate_out.h —, the rest queue and even out streams of unequal length)
   if (C.hist_len)
      ZH_LAUNCH(zh_inflate_streams_dict, grid, ZH_INFLATE_THREADS, 0, C.s8, (uint64_t)src_size, C.d8, (uint64_t)dst_size, C.hist + C.hist_len, C.hist_len, d_items, n, C.d_results);
   else
      ZH_LAUNCH(zh_inflate_streams, grid, ZH_INFLATE_THREADS, 0, C.s8, (uint64_t)src_size, C.d8, (uint64_t)dst_size, d_items, n, C.d_results);
   return 0;
}
// 4. the count of failed items; and of a host dst the out_size bytes of every item, and nothing between or behind them. C.order: the items in destination
// order (disjoint). Where every one filled its range and the ranges are adjacent, the span they cover is copied straight into dst; else it comes back in one
// copy and the items' bytes are taken out of it. R: zultra_hip_inflate_result_t or zultra_hip_member_result_t.
template <typename R>
static int zh_inflate_collect(const zh_inflate_call_t &C, void *dst, int dst_on_device, const zultra_hip_inflate_item_t *items, uint32_t n, const R *results) {
   int bad = 0;
   for (uint32_t k = 0; k < n; k++) {
      if (results[k].reason != 0) bad++;
      if (results[k].out_size > items[k].dst_cap) return -1;   // (the kernel checks every store: never)
   }
   if (dst_on_device || C.order.empty()) return bad;
   const uint64_t lo = items[C.order.front()].dst_off, hi = items[C.order.back()].dst_off + items[C.order.back()].dst_cap;
   uint64_t at = lo;
   bool whole = true;   // no byte of the span that an item has not written
   for (uint32_t k : C.order) {
      whole = whole && items[k].dst_off == at && results[k].out_size == items[k].dst_cap;
      at = items[k].dst_off + items[k].dst_cap;
   }
   std::vector<uint8_t> span(whole ? 0 : (size_t)(hi - lo));
   ZH_TRY(hipMemcpy(whole ? (uint8_t *)dst + lo : span.data(), C.d8 + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost));
   if (!whole)
      for (uint32_t k : C.order) memcpy((uint8_t *)dst + items[k].dst_off, span.data() + (items[k].dst_off - lo), (size_t)results[k].out_size);
   return bad;
}

// Many raw deflate streams, one wave each, with one preset dictionary for all items (dict_size 0: none).
extern "C" int zultra_hip_inflate_streams_dict(int device, const void *src, size_t src_size, int src_on_device, void *dst, size_t dst_size, int dst_on_device, const void *dict, size_t dict_size,
                                               int dict_on_device, const zultra_hip_inflate_item_t *items, uint32_t n, zultra_hip_inflate_result_t *results, float *kernel_ms) {
   ZH_EMU_SERIALIZE();
   if (kernel_ms) *kernel_ms = 0.f;
   zh_inflate_call_t C;
   if (zh_inflate_args(C, device, src, src_size, dst, dst_size, dst_on_device, dict, dict_size, dict_on_device, items, n, results)) return -1;
   if (zh_inflate_stage(C, device, src, src_size, src_on_device, dst, dst_size, dst_on_device, dict_on_device, items, n, ZH_IEV_INFLATE, ZH_IEV_CHECKS)) return -1;
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_INFLATE], 0));
   if (zh_inflate_launch(C, device, src_size, dst_size, C.d_items, n)) return -1;
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_CHECKS], 0));
   ZH_TRY(hipMemcpy(results, C.d_results, (size_t)n * sizeof(zh_inflate_result_t), hipMemcpyDeviceToHost));
   ZH_TRY(hipDeviceSynchronize());
   ZH_TRY(hipGetLastError());
   if (kernel_ms) (void)hipEventElapsedTime(kernel_ms, C.ev[ZH_IEV_INFLATE], C.ev[ZH_IEV_CHECKS]);
   return zh_inflate_collect(C, dst, dst_on_device, items, n, results);
}
extern "C" int zultra_hip_inflate_streams(int device, const void *src, size_t src_size, int src_on_device, void *dst, size_t dst_size, int dst_on_device,
                                          const zultra_hip_inflate_item_t *items, uint32_t n, zultra_hip_inflate_result_t *results, float *kernel_ms) {
   return zultra_hip_inflate_streams_dict(device, src, src_size, src_on_device, dst, dst_size, dst_on_device, NULL, 0, 0, items, n, results, kernel_ms);
}

// Adler-32 of a host buffer (the DICTID of a host dictionary)
static uint32_t zh_adler32_host(const uint8_t *p, size_t n) {
   uint32_t a = 1, b = 0;
   while (n) {
      const size_t run = n < 5552 ? n : 5552;   // (the longest run whose sums stay below 2^32)
      for (size_t i = 0; i < run; i++) {
         a += p[i];
         b += a;
      }
      a %= ZH_CK_ADLER_MOD;
      b %= ZH_CK_ADLER_MOD;
      p += run;
      n -= run;
   }
   return (b << 16) | a;
}

// zh_check_members' tables: the CRC-32 byte table, "append ZH_CK_SLICE zero bytes" and "append 64 * ZH_CK_SLICE zero bytes", the operators one table per state byte
static const std::vector<uint32_t> &zh_ck_tables() {
   static const std::vector<uint32_t> tables = [] {
      std::vector<uint32_t> t(ZH_CK_TABLE_WORDS);
      for (uint32_t i = 0; i < 256; i++) {
         uint32_t v = i;
         for (int k = 0; k < 8; k++) v = (v >> 1) ^ ((v & 1) ? 0xEDB88320u : 0);
         t[i] = v;
      }
      for (int b = 0; b < 4; b++)
         for (uint32_t i = 0; i < 256; i++) {
            uint32_t v = i << (8 * b);
            for (uint32_t k = 0; k < ZH_CK_SLICE; k++) v = (v >> 8) ^ t[v & 0xff];
            t[256 + 256 * b + i] = v;
         }
      for (int b = 0; b < 4; b++)
         for (uint32_t i = 0; i < 256; i++) {
            uint32_t v = i << (8 * b);
            for (int k = 0; k < 64; k++) v = t[256 + (v & 0xff)] ^ t[512 + ((v >> 8) & 0xff)] ^ t[768 + ((v >> 16) & 0xff)] ^ t[1024 + (v >> 24)];
            t[1280 + 256 * b + i] = v;
         }
      return t;
   }();
   return tables;
}

// zh_check_members<framing> over n items: idx = those of at most ZH_CK_SMALL_MAX bytes of room first (spg threads each), then the others
static int zh_check_launch(uint32_t framing, const uint8_t *src, const uint8_t *dst, uint64_t dst_size, const zh_inflate_item_t *d_items, const zh_inflate_result_t *d_inner,
                           zh_member_result_t *d_members, const uint32_t *d_idx, uint32_t nsmall, uint32_t nlarge, uint32_t spg, const uint32_t *d_tables,
                           const zh_zip_dirent_t *d_dirents = NULL /* ZH_M_ZIP: in the place of d_items */) {
   uint32_t small_blocks, large_blocks = nlarge;
   if (framing == ZH_M_RAW) {
      small_blocks = (uint32_t)zh_min64(((uint64_t)nsmall + nlarge + ZH_CK_THREADS - 1) / ZH_CK_THREADS, 4096);
      large_blocks = 0;
   }
   else
      small_blocks = (nsmall + ZH_CK_THREADS / spg - 1) / (ZH_CK_THREADS / spg);
   const uint32_t grid_cap = zh_grid_cap();   // (half of it for either form)
   if (grid_cap) {
      small_blocks = min(small_blocks, max(1u, grid_cap / 2));
      large_blocks = min(large_blocks, max(1u, grid_cap - grid_cap / 2));
   }
   decltype(&zh_check_members<ZH_M_RAW>) check_members = zh_check_members<ZH_M_RAW>;
   switch (framing) {
   case ZH_M_GZIP: check_members = zh_check_members<ZH_M_GZIP>; break;
   case ZH_M_ZLIB: check_members = zh_check_members<ZH_M_ZLIB>; break;
   case ZH_M_ZIP: check_members = zh_check_members<ZH_M_ZIP>; break;
   }
   ZH_LAUNCH(check_members, small_blocks + large_blocks, ZH_CK_THREADS, 0, src, dst, dst_size, d_items, d_inner, d_members, d_idx, nsmall, nlarge, spg, small_blocks, d_tables, d_dirents);
   return 0;
}

// The checksum kernel's two forms: by the room an item has (what it will have written is known on the device only). Uploads idx and, for the CRC-32, the tables.
static int zh_check_plan(zh_inflate_call_t &C, const zultra_hip_inflate_item_t *items, uint32_t n, unsigned int framing) {
   std::vector<uint32_t> idx(n);
   for (uint32_t k = 0; k < n; k++)
      if (items[k].dst_cap <= ZH_CK_SMALL_MAX) {
         idx[C.nsmall++] = k;
         while ((uint64_t)C.spg * ZH_CK_SLICE < items[k].dst_cap) C.spg *= 2;
      }
   for (uint32_t k = 0; k < n; k++)
      if (items[k].dst_cap > ZH_CK_SMALL_MAX) idx[C.nsmall + C.nlarge++] = k;
   ZH_TRY(zh_dalloc(&C.d_idx, n));
   ZH_TRY(hipMemcpy(C.d_idx, idx.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
   if (framing == ZH_M_GZIP || framing == ZH_M_ZIP) {
      ZH_TRY(zh_dalloc(&C.d_tables, ZH_CK_TABLE_WORDS));
      ZH_TRY(hipMemcpy(C.d_tables, zh_ck_tables().data(), ZH_CK_TABLE_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice));
   }
   return 0;
}

// DICTID (zlib): the Adler-32 of the WHOLE dictionary, once per call — the host's sum of a host dictionary; of a device dictionary the checksum kernel's, as
// a batch of one item whose "output" is the dictionary (no trailer behind it: its reason is not looked at, its `check` is).
// -> where zh_frame_heads reads the sum (it does so only for zlib items of a call with a dictionary), NULL if a step failed
static const zh_member_result_t *zh_dictid(zh_inflate_call_t &C, unsigned int framing, const void *dict, size_t dict_size, int dict_on_device) {
   if (zh_dalloc(&C.d_dictjob, 1) != hipSuccess) return NULL;
   zh_dictjob_t *const dj = C.d_dictjob;
   if (framing != ZH_M_ZLIB || dict_size == 0) return &dj->member;
   zh_dictjob_t job = {};
   job.item.dst_cap = job.inner.out_size = dict_size;
   if (!dict_on_device) job.member.check = zh_adler32_host((const uint8_t *)dict, dict_size);
   if (hipMemcpy(dj, &job, sizeof(job), hipMemcpyHostToDevice) != hipSuccess) return NULL;
   const bool small = dict_size <= ZH_CK_SMALL_MAX;
   if (dict_on_device && zh_check_launch(ZH_M_ZLIB, (const uint8_t *)dict, (const uint8_t *)dict, dict_size, &dj->item, &dj->inner, &dj->member, &dj->idx, small ? 1 : 0, small ? 0 : 1,
                                         ZH_CK_SMALL_MAX / ZH_CK_SLICE, NULL))
      return NULL;
   return &dj->member;
}

// 5. the members of a call whose n items lie in C.d_items (`items`: the host's copy of them): headers, inflate, checksums and trailers in three launches
// on the null stream, between the call's events HEADS .. END. dst_size: what the kernels are told of the destination; dict: the whole dictionary (dict_size 0:
// none; zh_inflate_args has taken its history); with_dictid: zh_frame_heads gets a DICTID to compare with (a call that takes a dictionary: a whole file does not).
static int zh_members_enqueue(zh_inflate_call_t &C, int device, size_t src_size, size_t dst_size, unsigned int framing, bool with_dictid, const void *dict, size_t dict_size, int dict_on_device,
                              const zultra_hip_inflate_item_t *items, uint32_t n) {
   ZH_TRY(zh_dalloc(&C.d_inner, n));
   ZH_TRY(zh_dalloc(&C.d_members, n));
   if (zh_check_plan(C, items, n, framing)) return -1;
   const zh_member_result_t *d_dictsum = NULL;
   if (with_dictid && !(d_dictsum = zh_dictid(C, framing, dict, dict_size, dict_on_device))) return -1;
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_HEADS], 0));
   ZH_LAUNCH(zh_frame_heads, (uint32_t)zh_min64(((uint64_t)n + ZH_FRAME_THREADS - 1) / ZH_FRAME_THREADS, 4096), ZH_FRAME_THREADS, 0, C.s8, (uint64_t)src_size, C.d_items, n, (uint32_t)framing,
             dict_size ? 1u : 0u, d_dictsum, C.d_inner, C.d_members);
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_INFLATE], 0));
   if (zh_inflate_launch(C, device, src_size, dst_size, C.d_inner, n)) return -1;
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_CHECKS], 0));
   if (zh_check_launch(framing, C.s8, C.d8, dst_size, C.d_items, C.d_results, C.d_members, C.d_idx, C.nsmall, C.nlarge, C.spg, C.d_tables)) return -1;
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_END], 0));
   return 0;
}
// 6. ... their results read back, the call's one synchronisation; ms: the three kernel times
static int zh_members_collect(const zh_inflate_call_t &C, uint32_t n, zultra_hip_member_result_t *results, float *ms) {
   ZH_TRY(hipMemcpy(results, C.d_members, (size_t)n * sizeof(zh_member_result_t), hipMemcpyDeviceToHost));
   ZH_TRY(hipDeviceSynchronize());
   ZH_TRY(hipGetLastError());
   if (ms)
      for (int i = 0; i < 3; i++) (void)hipEventElapsedTime(ms + i, C.ev[ZH_IEV_HEADS + i], C.ev[ZH_IEV_HEADS + i + 1]);
   return 0;
}
static int zh_members_run(zh_inflate_call_t &C, int device, size_t src_size, size_t dst_size, unsigned int framing, bool with_dictid, const void *dict, size_t dict_size, int dict_on_device,
                          const zultra_hip_inflate_item_t *items, uint32_t n, zultra_hip_member_result_t *results, float *ms) {
   if (zh_members_enqueue(C, device, src_size, dst_size, framing, with_dictid, dict, dict_size, dict_on_device, items, n)) return -1;
   return zh_members_collect(C, n, results, ms);
}

// Many gzip / zlib members (or raw streams).
extern "C" int zultra_hip_inflate_members(int device, const void *src, size_t src_size, int src_on_device, void *dst, size_t dst_size, int dst_on_device, const void *dict, size_t dict_size,
                                          int dict_on_device, unsigned int framing, const zultra_hip_inflate_item_t *items, uint32_t n, zultra_hip_member_result_t *results, float *kernel_ms) {
   ZH_EMU_SERIALIZE();
   if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0.f;
   if (framing != ZH_M_RAW && framing != ZH_M_ZLIB && framing != ZH_M_GZIP) return -1;
   zh_inflate_call_t C;
   if (zh_inflate_args(C, device, src, src_size, dst, dst_size, dst_on_device, dict, dict_size, dict_on_device, items, n, results)) return -1;
   if (zh_inflate_stage(C, device, src, src_size, src_on_device, dst, dst_size, dst_on_device, dict_on_device, items, n, ZH_IEV_HEADS, ZH_IEV_END)) return -1;
   if (zh_members_run(C, device, src_size, dst_size, framing, true, dict, dict_size, dict_on_device, items, n, results, kernel_ms)) return -1;
   return zh_inflate_collect(C, dst, dst_on_device, items, n, results);
}

// ---- the member index of a whole file (zh_inflate_index.h) -------------------------------------------------------------------------------------------
static_assert(sizeof(zh_ix_tile_t) == 64, "one record per tile");

// what the calls below keep of an index between its passes. zip: the records are a ZIP archive's central directory (zh_unzip.h), else gzip members; D0, size:
// the range of the source that the chain runs over (gzip members: the whole source)
struct zh_index_t {
   bool zip = false;
   uint64_t D0 = 0, size = 0;
   uint64_t D1 = 0, T = 0, ntiles = 0;   // (zh_index_run)
   zh_ix_totals_t tot = {};
};
// 1. the arguments, the device, the index's four events and the events `first` to `last` (first > last: none), the source staged; the format's tile and resolve
// kernels between the index's two events; the totals read back (the call's first synchronisation) into X.tot
static int zh_index_run(zh_inflate_call_t &C, zh_index_t &X, int device, const void *src, size_t src_size, int src_on_device, int first, int last) {
   if (!src || src_size == 0 || X.D0 > src_size || X.size > src_size - X.D0 || device < 0 || device >= zultra_hip_device_count()) return -1;
   X.D1 = X.D0 + X.size;
   ZH_TRY(hipSetDevice(device));
   for (int e = ZH_IEV_INDEX_START; e <= ZH_IEV_ITEMS_END; e++) ZH_TRY(hipEventCreate(&C.ev[e]));
   for (int e = first; e <= last; e++) ZH_TRY(hipEventCreate(&C.ev[e]));
   C.s8 = (const uint8_t *)src;
   if (!src_on_device) {
      ZH_TRY(zh_dalloc(&C.d_src, src_size));
      ZH_TRY(hipMemcpy(C.d_src, src, src_size, hipMemcpyHostToDevice));
      C.s8 = C.d_src;
   }
   const int tile = zh_env("ZULTRA_HIP_INDEX_TILE", 0);   // tests, tools/inflate_time.py, tools/unzip_time.py: any value >= 32, no power of two needed
   X.T = tile >= (int)ZH_IX_TILE_MIN ? (uint64_t)tile : X.zip ? (uint64_t)ZH_UZ_TILE : (uint64_t)ZH_IX_TILE;
   X.ntiles = (X.size + X.T - 1) / X.T;   // (0: an empty directory, which the resolve pass alone reports)
   ZH_TRY(zh_dalloc(&C.d_ix_tiles, (size_t)zh_max64(X.ntiles, 1)));
   ZH_TRY(zh_dalloc(&C.d_ix_totals, 1));
   const uint32_t grid = zh_capped((uint32_t)zh_min64(zh_max64(X.ntiles, 1), 32ull * zh_device_cus(device)), zh_grid_cap());   // (one wave per workgroup, as the inflate kernel)
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_INDEX_START], 0));
   if (X.zip) {
      if (X.ntiles) ZH_LAUNCH(zh_uz_tiles, grid, ZH_IX_THREADS, 0, C.s8, (uint64_t)src_size, X.D0, X.D1, X.T, X.ntiles, C.d_ix_tiles);
      ZH_LAUNCH(zh_uz_resolve, 1, ZH_IX_THREADS, 0, C.s8, X.D0, X.D1, X.T, X.ntiles, C.d_ix_tiles, C.d_ix_totals);
   }
   else {
      ZH_LAUNCH(zh_ix_tiles, grid, ZH_IX_THREADS, 0, C.s8, (uint64_t)src_size, X.T, X.ntiles, C.d_ix_tiles);
      ZH_LAUNCH(zh_ix_resolve, 1, ZH_IX_THREADS, 0, C.s8, (uint64_t)src_size, X.T, X.ntiles, C.d_ix_tiles, C.d_ix_totals);
   }
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_INDEX_END], 0));
   ZH_TRY(hipMemcpy(&X.tot, C.d_ix_totals, sizeof(X.tot), hipMemcpyDeviceToHost));
   ZH_TRY(hipGetLastError());
   return 0;
}
// the totals as the two public result records name them
static void zh_index_report(const zh_index_t &X, zultra_hip_index_result_t *res) {
   res->members = (uint32_t)zh_min64(X.tot.members, 0xFFFFFFFFull);
   res->stop = X.tot.stop;
   res->out_size = X.tot.out_size;
   res->src_used = X.tot.src_used;
   res->tiles = (uint32_t)zh_min64(X.tot.tiles, 0xFFFFFFFFull);
   res->tiles_rewalked = (uint32_t)zh_min64(X.tot.tiles_rewalked, 0xFFFFFFFFull);
}
static void zh_index_report(const zh_index_t &X, zultra_hip_zip_index_result_t *res) {
   res->entries = (uint32_t)zh_min64(X.tot.members, 0xFFFFFFFFull);
   res->stop = X.tot.stop;
   res->out_size = X.tot.out_size;
   res->dir_used = X.tot.src_used - X.D0;
   res->tiles = (uint32_t)zh_min64(X.tot.tiles, 0xFFFFFFFFull);
   res->tiles_rewalked = (uint32_t)zh_min64(X.tot.tiles_rewalked, 0xFFFFFFFFull);
}
// 2. the format's items kernel into C.d_items or C.d_dirents (the index's count of them), between the items' two events
static int zh_index_items(zh_inflate_call_t &C, const zh_index_t &X) {
   ZH_TRY(X.zip ? zh_dalloc(&C.d_dirents, (size_t)X.tot.members) : zh_dalloc(&C.d_items, (size_t)X.tot.members));
   const uint32_t grid = zh_capped((uint32_t)zh_min64((X.ntiles + ZH_IX_THREADS - 1) / ZH_IX_THREADS, 4096), zh_grid_cap());
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_ITEMS_START], 0));
   if (X.zip) {
      ZH_LAUNCH(zh_uz_entries, grid, ZH_IX_THREADS, 0, C.s8, X.D0, X.D1, X.T, X.ntiles, C.d_ix_tiles, C.d_dirents);
   }
   else {
      ZH_LAUNCH(zh_ix_items, grid, ZH_IX_THREADS, 0, C.s8, X.D1, X.T, X.ntiles, C.d_ix_tiles, C.d_items);
   }
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_ITEMS_END], 0));
   return 0;
}
static float zh_index_ms(const zh_inflate_call_t &C, bool with_items) {
   float a = 0.f, b = 0.f;
   (void)hipEventElapsedTime(&a, C.ev[ZH_IEV_INDEX_START], C.ev[ZH_IEV_INDEX_END]);
   if (with_items) (void)hipEventElapsedTime(&b, C.ev[ZH_IEV_ITEMS_START], C.ev[ZH_IEV_ITEMS_END]);
   return a + b;
}

// The index alone.
extern "C" int zultra_hip_index_members(int device, const void *src, size_t src_size, int src_on_device, zultra_hip_inflate_item_t *items, uint32_t cap, zultra_hip_index_result_t *res,
                                        float *kernel_ms) {
   ZH_EMU_SERIALIZE();
   if (kernel_ms) *kernel_ms = 0.f;
   if (!res || (!items && cap)) return -1;
   memset(res, 0, sizeof(*res));
   zh_inflate_call_t C;
   zh_index_t X;
   X.size = src_size;
   if (zh_index_run(C, X, device, src, src_size, src_on_device, 0, -1)) return -1;
   zh_index_report(X, res);
   const bool want = items != NULL && cap != 0;
   if (X.tot.members > 0xFFFFFFFFull || (want && X.tot.members > cap)) {
      res->stop = 4;
      return -1;
   }
   const bool with_items = want && X.tot.members != 0;
   if (with_items) {
      if (zh_index_items(C, X)) return -1;
      ZH_TRY(hipMemcpy(items, C.d_items, (size_t)X.tot.members * sizeof(zh_inflate_item_t), hipMemcpyDeviceToHost));
   }
   ZH_TRY(hipDeviceSynchronize());
   ZH_TRY(hipGetLastError());
   if (kernel_ms) *kernel_ms = zh_index_ms(C, with_items);
   return 0;
}

// A whole file: the index, then the members of zultra_hip_inflate_members over the items where the index left them, in device memory. The index makes
// the destination ranges disjoint, in order and in range, so nothing is sorted here; the host reads the items once, for the checksum kernel's two forms.
extern "C" int zultra_hip_inflate_file(int device, const void *src, size_t src_size, int src_on_device, void *dst, size_t dst_size, int dst_on_device, zultra_hip_index_result_t *res,
                                       zultra_hip_member_result_t *results, uint32_t results_cap, float *kernel_ms) {
   ZH_EMU_SERIALIZE();
   if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = kernel_ms[3] = 0.f;
   if (!res || !dst) return -1;
   memset(res, 0, sizeof(*res));
   zh_inflate_call_t C;
   zh_index_t X;
   X.size = src_size;
   if (zh_index_run(C, X, device, src, src_size, src_on_device, ZH_IEV_HEADS, ZH_IEV_END)) return -1;
   zh_index_report(X, res);
   if (X.tot.members > 0xFFFFFFFFull || X.tot.out_size > dst_size || (results && X.tot.members > results_cap)) {
      res->stop = 4;   // nothing is decoded: res says how much room the file needs
      return -1;
   }
   const uint32_t n = (uint32_t)X.tot.members;
   if (n == 0) {
      if (kernel_ms) kernel_ms[0] = zh_index_ms(C, false);
      return 0;
   }
   const size_t out_size = (size_t)X.tot.out_size;
   if (zh_index_items(C, X)) return -1;
   std::vector<zultra_hip_inflate_item_t> items(n);
   ZH_TRY(hipMemcpy(items.data(), C.d_items, (size_t)n * sizeof(zh_inflate_item_t), hipMemcpyDeviceToHost));
   ZH_TRY(hipGetLastError());
   C.d8 = (uint8_t *)dst;
   if (!dst_on_device) {   // a host destination is staged: exactly the bytes the index counted
      ZH_TRY(zh_dalloc(&C.d_dst, out_size ? out_size : 1));
      C.d8 = C.d_dst;
   }
   ZH_TRY(zh_dalloc(&C.d_results, n));
   std::vector<zultra_hip_member_result_t> own;
   if (!results) {
      own.resize(n);
      results = own.data();
   }
   if (zh_members_run(C, device, src_size, dst_on_device ? dst_size : out_size, ZH_M_GZIP, false, NULL, 0, 0, items.data(), n, results, kernel_ms ? kernel_ms + 1 : NULL)) return -1;
   if (kernel_ms) kernel_ms[0] = zh_index_ms(C, true);
   C.order.reserve(n);
   for (uint32_t k = 0; k < n; k++)   // (as the index put them)
      if (items[k].dst_cap) C.order.push_back(k);
   return zh_inflate_collect(C, dst, dst_on_device, items.data(), n, results);
}

// ---- a byte range of a whole file (zh_inflate_range.h) ---------------------------------------------------------------------------------------------------
static void zh_index_report(const zh_index_t &X, zultra_hip_range_result_t *res) {
   res->members = (uint32_t)zh_min64(X.tot.members, 0xFFFFFFFFull);
   res->stop = X.tot.stop;
   res->file_size = X.tot.out_size;
   res->src_used = X.tot.src_used;
   res->tiles = (uint32_t)zh_min64(X.tot.tiles, 0xFFFFFFFFull);
   res->tiles_rewalked = (uint32_t)zh_min64(X.tot.tiles_rewalked, 0xFFFFFFFFull);
}

// Bytes [first, first + nbytes) of the indexed members' output: the index; the two members that hold the ends of the range picked from the tile records (the
// plan, read back with the room checks); the items of members m0 .. m1, those wholly inside the range rebased to it, the one or two that straddle an end sent
// to the edge buffer; ONE batch through the three launches — its destination the lower of the two buffers' addresses, so that every member of the range is
// in flight at once —; the slices moved out of the edge buffer; the results read back behind one synchronisation.
extern "C" int zultra_hip_inflate_range(int device, const void *src, size_t src_size, int src_on_device, uint64_t first, uint64_t nbytes, void *dst, size_t dst_size, int dst_on_device,
                                        zultra_hip_range_result_t *res, zultra_hip_member_result_t *results, uint32_t results_cap, float *kernel_ms) {
   ZH_EMU_SERIALIZE();
   if (kernel_ms)
      for (int i = 0; i < 5; i++) kernel_ms[i] = 0.f;
   if (!res || !dst) return -1;
   memset(res, 0, sizeof(*res));
   zh_inflate_call_t C;
   zh_index_t X;
   X.size = src_size;
   if (zh_index_run(C, X, device, src, src_size, src_on_device, ZH_IEV_HEADS, ZH_IEV_RG_END)) return -1;
   zh_index_report(X, res);
   const uint64_t F = X.tot.out_size, lo = zh_min64(first, F), hi = zh_min64(nbytes > ~0ull - first ? ~0ull : first + nbytes, F);
   res->out_size = hi - lo;
   if (hi == lo) {   // nothing of the range exists: nothing is decoded
      ZH_TRY(hipDeviceSynchronize());
      if (kernel_ms) kernel_ms[0] = zh_index_ms(C, false);
      return 0;
   }
   // the plan
   ZH_TRY(zh_dalloc(&C.d_plan, 1));
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_ITEMS_START], 0));
   ZH_LAUNCH(zh_rg_select, 1, ZH_RG_THREADS, 0, C.s8, (uint64_t)src_size, X.ntiles, C.d_ix_tiles, lo, hi - 1u, C.d_plan);
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_RG_PLAN], 0));
   zh_rg_plan_t plan;
   ZH_TRY(hipMemcpy(&plan, C.d_plan, sizeof(plan), hipMemcpyDeviceToHost));
   ZH_TRY(hipGetLastError());
   const zh_rg_end_t &a = plan.end[0], &b = plan.end[1];
   if (!a.found || !b.found || b.member < a.member || b.tile < a.tile || b.tile >= X.ntiles) return -1;   // (never: the index holds every byte below F)
   const uint64_t count = b.member - a.member + 1u;
   res->first_member = (uint32_t)zh_min64(a.member, 0xFFFFFFFFull);
   res->range_members = (uint32_t)zh_min64(count, 0xFFFFFFFFull);
   if (a.member > 0xFFFFFFFFull || count > 0xFFFFFFFFull || hi - lo > dst_size || (results && count > results_cap)) {
      res->stop = 4;   // nothing is decoded: res says how much room the range needs
      return -1;
   }
   const uint32_t n = (uint32_t)count;
   const size_t out_size = (size_t)(hi - lo);
   // the members that straddle an end: decoded in full into the edge buffer, the head's at 0, the tail's behind it, both 16-byte aligned
   const bool one = a.member == b.member;
   const bool head_edge = a.out_off < lo || a.out_off + a.isize > hi, tail_edge = !one && b.out_off + b.isize > hi;
   const uint64_t tail_at = head_edge ? ((uint64_t)a.isize + 15u) & ~15ull : 0u, edge_room = tail_at + (tail_edge ? ((uint64_t)b.isize + 15u) & ~15ull : 0u);
   // the two buffers: a host destination is staged behind the edge buffer in one allocation, exactly the bytes of the range
   uint8_t *range8 = (uint8_t *)dst, *edge8 = NULL;
   if (!dst_on_device) {
      ZH_TRY(zh_dalloc(&C.d_dst, (size_t)edge_room + out_size));
      edge8 = C.d_dst;
      range8 = C.d_dst + edge_room;
   }
   else if (edge_room) {
      ZH_TRY(zh_dalloc(&C.d_edge, (size_t)edge_room));
      edge8 = C.d_edge;
   }
   // ... as one destination for the three launches: from the lower address to the end of the higher buffer
   C.d8 = edge_room && edge8 < range8 ? edge8 : range8;
   const uint64_t range_at = (uint64_t)(range8 - C.d8), edge_at = edge_room ? (uint64_t)(edge8 - C.d8) : 0u;
   const size_t span = (size_t)zh_max64(range_at + out_size, edge_at + edge_room);
   zh_rg_edge_t head = {}, tail = {};
   if (head_edge) {
      head.buf_at = 0;
      head.from = lo - a.out_off;   // (the member holds byte lo)
      head.to = zh_min64(hi - a.out_off, a.isize);
      head.dst_at = 0;
      head.slot = 0;
   }
   if (tail_edge) {
      tail.buf_at = tail_at;
      tail.from = 0;
      tail.to = hi - b.out_off;
      tail.dst_at = b.out_off - lo;
      tail.slot = n - 1u;
   }
   // the items, where the three launches read them; the host's copy of them for the checksum kernel's two forms: 32 bytes per member of the range
   ZH_TRY(zh_dalloc(&C.d_items, n));
   const uint64_t ntiles = b.tile - a.tile + 1u;
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_RG_ITEMS], 0));
   ZH_LAUNCH(zh_rg_items, zh_capped((uint32_t)zh_min64((ntiles + ZH_RG_THREADS - 1) / ZH_RG_THREADS, 4096), zh_grid_cap()), ZH_RG_THREADS, 0, C.s8, (uint64_t)src_size, C.d_ix_tiles, a.tile,
             b.tile, a.member, b.member, lo, hi, range_at, edge_at, edge_at + tail_at, C.d_items);
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_ITEMS_END], 0));
   std::vector<zultra_hip_inflate_item_t> items(n);
   ZH_TRY(hipMemcpy(items.data(), C.d_items, (size_t)n * sizeof(zh_inflate_item_t), hipMemcpyDeviceToHost));
   ZH_TRY(hipGetLastError());
   std::vector<zultra_hip_member_result_t> own;
   if (!results) {
      own.resize(n);
      results = own.data();
   }
   ZH_TRY(zh_dalloc(&C.d_results, n));
   if (zh_members_enqueue(C, device, src_size, span, ZH_M_GZIP, false, NULL, 0, 0, items.data(), n)) return -1;
   if (head_edge || tail_edge) {   // a wave per edge and slice, as many slices as the longer edge has
      const uint64_t longest = zh_max64(head.to - head.from, tail.to - tail.from);
      uint32_t yslices = (uint32_t)zh_min64(zh_max64((longest / 16 + ZH_ZIP_SLICE_CHUNKS - 1) / ZH_ZIP_SLICE_CHUNKS, 1), ZH_RG_MAX_YSLICES);
      if (zh_grid_cap()) yslices = max(1u, min(yslices, zh_grid_cap() / 2));
      ZH_LAUNCH(zh_rg_edges, 2 * yslices, ZH_RG_THREADS, 0, edge8, edge_room, range8, head, tail, C.d_members, yslices);
   }
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_RG_END], 0));
   if (zh_members_collect(C, n, results, kernel_ms ? kernel_ms + 2 : NULL)) return -1;
   if (kernel_ms) {
      kernel_ms[0] = zh_index_ms(C, false);
      float select = 0.f, fill = 0.f, edges = 0.f;
      (void)hipEventElapsedTime(&select, C.ev[ZH_IEV_ITEMS_START], C.ev[ZH_IEV_RG_PLAN]);
      (void)hipEventElapsedTime(&fill, C.ev[ZH_IEV_RG_ITEMS], C.ev[ZH_IEV_ITEMS_END]);
      (void)hipEventElapsedTime(&edges, C.ev[ZH_IEV_END], C.ev[ZH_IEV_RG_END]);
      kernel_ms[1] = select + fill;
      kernel_ms[4] += edges;
   }
   int bad = 0;
   for (uint32_t k = 0; k < n; k++)
      if (results[k].reason != 0) bad++;
   if (!dst_on_device) ZH_TRY(hipMemcpy(dst, range8, out_size, hipMemcpyDeviceToHost));
   return bad;
}

// ---- a ZIP archive read (zh_unzip.h) ------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(zultra_hip_zip_dirent_t) == sizeof(zh_zip_dirent_t) && sizeof(zh_zip_dirent_t) == 48, "ABI");

// The directory index alone.
extern "C" int zultra_hip_zip_index(int device, const void *src, size_t src_size, int src_on_device, uint64_t central_at, uint64_t central_size, zultra_hip_zip_dirent_t *dirents, uint32_t cap,
                                    zultra_hip_zip_index_result_t *res, float *kernel_ms) {
   ZH_EMU_SERIALIZE();
   if (kernel_ms) *kernel_ms = 0.f;
   if (!res || (!dirents && cap)) return -1;
   memset(res, 0, sizeof(*res));
   zh_inflate_call_t C;
   zh_index_t X;
   X.zip = true, X.D0 = central_at, X.size = central_size;
   if (zh_index_run(C, X, device, src, src_size, src_on_device, 0, -1)) return -1;
   zh_index_report(X, res);
   const bool want = dirents != NULL && cap != 0;
   if (X.tot.members > 0xFFFFFFFFull || (want && X.tot.members > cap)) {
      res->stop = 4;
      return -1;
   }
   const bool with_items = want && X.tot.members != 0;
   if (with_items) {
      if (zh_index_items(C, X)) return -1;
      ZH_TRY(hipMemcpy(dirents, C.d_dirents, (size_t)X.tot.members * sizeof(zh_zip_dirent_t), hipMemcpyDeviceToHost));
   }
   ZH_TRY(hipDeviceSynchronize());
   ZH_TRY(hipGetLastError());
   if (kernel_ms) *kernel_ms = zh_index_ms(C, with_items);
   return 0;
}

// A whole archive: the index; the dirents read once, for the checksum kernel's two forms and the copy kernel's grid; then local headers, inflate, copy and
// checks in four launches on the null stream, the results read back, one synchronisation at the end. The index makes the destination ranges disjoint, in order
// and — behind the out_size gate — in range.
extern "C" int zultra_hip_unzip(int device, const void *src, size_t src_size, int src_on_device, uint64_t central_at, uint64_t central_size, int64_t local_delta, void *dst, size_t dst_size,
                                int dst_on_device, zultra_hip_zip_index_result_t *res, zultra_hip_zip_dirent_t *dirents, zultra_hip_member_result_t *results, uint32_t cap, float *kernel_ms) {
   ZH_EMU_SERIALIZE();
   if (kernel_ms)
      for (int i = 0; i < 5; i++) kernel_ms[i] = 0.f;
   if (!res || (!dst && dst_size) || local_delta > (1ll << 62) || local_delta < -(1ll << 62)) return -1;
   memset(res, 0, sizeof(*res));
   zh_inflate_call_t C;
   zh_index_t X;
   X.zip = true, X.D0 = central_at, X.size = central_size;
   if (zh_index_run(C, X, device, src, src_size, src_on_device, ZH_IEV_UZ_LOCALS, ZH_IEV_UZ_END)) return -1;
   zh_index_report(X, res);
   if (X.tot.stop == 1 || X.tot.stop == 2) return -1;   // nothing is decoded from a directory that does not end where it should
   if (X.tot.members > 0xFFFFFFFFull || X.tot.out_size > dst_size || ((dirents || results) && X.tot.members > cap)) {
      res->stop = 4;   // nothing is decoded: res says how much room the archive needs
      return -1;
   }
   const uint32_t n = (uint32_t)X.tot.members;
   if (n == 0) {
      if (kernel_ms) kernel_ms[0] = zh_index_ms(C, false);
      return 0;
   }
   const size_t out_size = (size_t)X.tot.out_size;
   if (zh_index_items(C, X)) return -1;
   std::vector<zultra_hip_zip_dirent_t> own_dirents;
   if (!dirents) {
      own_dirents.resize(n);
      dirents = own_dirents.data();
   }
   ZH_TRY(hipMemcpy(dirents, C.d_dirents, (size_t)n * sizeof(zh_zip_dirent_t), hipMemcpyDeviceToHost));
   ZH_TRY(hipGetLastError());
   // an entry's room as an item: what zh_check_plan splits by and zh_inflate_collect copies by; the stored entries that may be copied, and the largest of them
   std::vector<zultra_hip_inflate_item_t> items(n);
   uint32_t ncopy = 0, copy_max = 0;
   for (uint32_t k = 0; k < n; k++) {
      items[k] = {0, 0, dirents[k].dst_off, dirents[k].size};
      if (dirents[k].method == 0 && dirents[k].size && dirents[k].size != 0xFFFFFFFFu) {
         ncopy++;
         copy_max = std::max(copy_max, dirents[k].size);
      }
   }
   C.d8 = (uint8_t *)dst;
   if (!dst_on_device) {   // a host destination is staged: exactly the bytes the index counted
      ZH_TRY(zh_dalloc(&C.d_dst, out_size ? out_size : 1));
      C.d8 = C.d_dst;
   }
   const size_t room = dst_on_device ? dst_size : out_size;
   ZH_TRY(zh_dalloc(&C.d_inner, n));
   ZH_TRY(zh_dalloc(&C.d_results, n));
   ZH_TRY(zh_dalloc(&C.d_members, n));
   ZH_TRY(zh_dalloc(&C.d_copies, ncopy ? ncopy : 1));
   ZH_TRY(zh_dalloc(&C.d_ncopies, 1));
   ZH_TRY(hipMemset(C.d_ncopies, 0, sizeof(uint32_t)));
   if (zh_check_plan(C, items.data(), n, ZH_M_ZIP)) return -1;
   const uint32_t grid_cap = zh_grid_cap();
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_UZ_LOCALS], 0));
   ZH_LAUNCH(zh_uz_locals, zh_capped((uint32_t)zh_min64(((uint64_t)n + ZH_UZ_THREADS - 1) / ZH_UZ_THREADS, 4096), grid_cap), ZH_UZ_THREADS, 0, C.s8, (uint64_t)src_size, C.d_dirents, n,
             (int64_t)local_delta, C.d_inner, C.d_members, C.d_copies, C.d_ncopies);
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_UZ_INFLATE], 0));
   if (zh_inflate_launch(C, device, src_size, room, C.d_inner, n)) return -1;
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_UZ_COPY], 0));
   if (ncopy) {
      // a grid of a multiple of yslices workgroups, yslices by the largest stored entry (zh_zip_copy's layout)
      const uint32_t waves = ZH_UZ_COPY_THREADS / 64;
      uint32_t yslices = (uint32_t)zh_min64(zh_max64(((uint64_t)copy_max / 16 + ZH_ZIP_SLICE_CHUNKS - 1) / ZH_ZIP_SLICE_CHUNKS, 1), ZH_UZ_MAX_YSLICES);
      uint32_t xdim = (uint32_t)zh_min64(((uint64_t)ncopy + waves - 1) / waves, zh_max64(8ull * zh_device_cus(device) / yslices, 1));
      if (grid_cap) {
         yslices = min(yslices, grid_cap);
         xdim = max(1u, min(xdim, grid_cap / yslices));
      }
      ZH_LAUNCH(zh_uz_copy, xdim * yslices, ZH_UZ_COPY_THREADS, 0, C.s8, (uint64_t)src_size, C.d8, C.d_copies, C.d_ncopies, yslices);
   }
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_UZ_CHECKS], 0));
   if (zh_check_launch(ZH_M_ZIP, C.s8, C.d8, room, C.d_inner, C.d_results, C.d_members, C.d_idx, C.nsmall, C.nlarge, C.spg, C.d_tables, C.d_dirents)) return -1;
   ZH_TRY(hipEventRecord(C.ev[ZH_IEV_UZ_END], 0));
   std::vector<zultra_hip_member_result_t> own;
   if (!results) {
      own.resize(n);
      results = own.data();
   }
   ZH_TRY(hipMemcpy(results, C.d_members, (size_t)n * sizeof(zh_member_result_t), hipMemcpyDeviceToHost));
   ZH_TRY(hipDeviceSynchronize());
   ZH_TRY(hipGetLastError());
   if (kernel_ms) {
      kernel_ms[0] = zh_index_ms(C, true);
      for (int i = 0; i < 4; i++) (void)hipEventElapsedTime(kernel_ms + 1 + i, C.ev[ZH_IEV_UZ_LOCALS + i], C.ev[ZH_IEV_UZ_LOCALS + i + 1]);
   }
   C.order.reserve(n);
   for (uint32_t k = 0; k < n; k++)   // (as the index put them)
      if (items[k].dst_cap) C.order.push_back(k);
   return zh_inflate_collect(C, dst, dst_on_device, items.data(), n, results);
}

// For libzultra.cpp, which has no HIP of its own: a device copy of a host buffer, so that a call that walks a file run by run uploads it once.
extern "C" ZH_HIDDEN void *zh_device_upload(int device, const void *host, size_t n) {
   void *p = NULL;
   if (!host || n == 0 || device < 0 || device >= zultra_hip_device_count() || hipSetDevice(device) != hipSuccess || hipMalloc(&p, n) != hipSuccess) return NULL;
   if (hipMemcpy(p, host, n, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(p);
      return NULL;
   }
   return p;
}
extern "C" ZH_HIDDEN void zh_device_release(void *p) { (void)hipFree(p); }
