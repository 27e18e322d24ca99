// zh_zip.h — a ZIP archive's entries on the device: local headers, names and streams at their final byte offsets, and the central directory records.
//
// A gather behind the plain files-form assembly (zh_stitch.h), not room inside it: zh_stitch_scan has ONE head size per launch and a local header is
// 30 + name length bytes, another for every entry. So the stream buffer stays as the assembly left it — this header never writes it — and three kernels
// fill a second buffer: the LOCAL PART, entry after entry {local header, name, stream}, and behind it at a 16-byte aligned position
// the CENTRAL PART, {central header, name} per entry.
//   zh_zip_scan     one workgroup: the entries' local offsets (an exclusive prefix sum of 30 + name_len + comp_size over chunks of entries, with the
//                   chunks' sums scanned in LDS), comp_size from file_off, the two totals, the verdict
//   zh_zip_records  a lane per entry: the CRC-32 finalised from its linear part, the 30 and 46 bytes of headers and the name behind each
//   zh_zip_copy     the streams: 16-byte stores to aligned destinations, put together from aligned loads with a byte shift; the edges bytewise
// Who writes which byte: zh_zip_records writes the header and name bytes of its entry, zh_zip_copy the stream bytes of its (entry, slice) — whole
// 16-byte chunks only where all 16 bytes are the stream's, single bytes at the up to 15 on either edge, which share their dwords with the neighbouring
// records. No byte has two writers, nothing is read back, and the two kernels need no order between them.
// An empty entry (a zero-length file or a directory) has no max-block: method 0, sizes 0, CRC 0, version needed 10.
#pragma once
#include "zh_copy.h"
#include "zh_frame.h"

#define ZH_ZIP_EMPTY 0xFFFFFFFFu    // entry_block[i]: no max-block
#define ZH_ZIP_LOCAL 30u
#define ZH_ZIP_CENTRAL 46u
#define ZH_ZIP_LIMIT 0xFFFFFFFFull   // sizes and offsets from here on need ZIP64 fields per entry: refused

struct zh_zip_entry_t {   // = zultra_hip_zip_entry_t
   uint64_t local_off;    // of the local header in the archive: base_off + its position in the local part
   uint32_t comp_size, size, crc32, name_len;
};
struct zh_zip_report_t {
   uint64_t local_bytes, central_bytes;
   uint32_t failed;       // 1: the assembly in the stream buffer failed (zh_stitch's conditions); 2: the 32-bit limit. Nothing is written then
   uint32_t pad;
};

#if defined(__HIPCC__) || defined(ZH_EMU)

// chunk t of ceil(n / threads) entries belongs to thread t: summed, scanned over the threads, walked again from its start (zh_stitch_scan's carry)
#define ZH_ZIP_SCAN_THREADS 1024
__global__ void __launch_bounds__(ZH_ZIP_SCAN_THREADS)
zh_zip_scan(const uint32_t *__restrict__ name_off, const uint32_t *__restrict__ entry_block /* NULL: entry i = max-block i */, uint32_t n, const zh_block_t *__restrict__ blocks,
            const uint64_t *__restrict__ file_off, const zh_scan_out_t *__restrict__ scan, uint64_t stream_cap, uint64_t base_off,
            zh_zip_entry_t *entries, uint64_t *src_off /* per entry: first byte of its stream in the stream buffer; ~0: none */, zh_zip_report_t *report) {
   __shared__ uint64_t part[ZH_ZIP_SCAN_THREADS];
   const uint32_t tid = threadIdx.x, chunk = (n + ZH_ZIP_SCAN_THREADS - 1) / ZH_ZIP_SCAN_THREADS;
   const uint32_t lo = (uint32_t)min((uint64_t)n, (uint64_t)tid * chunk), hi = (uint32_t)min((uint64_t)n, (uint64_t)lo + chunk);
   const bool assembled = !scan->failed && !scan->oversize && ((scan->end_bit + 7) >> 3) + 8 <= stream_cap;   // (else file_off is not to be read)
   uint64_t sum = 0;
   if (assembled)
      for (uint32_t i = lo; i < hi; i++) {
         const uint32_t b = entry_block ? entry_block[i] : i;
         sum += ZH_ZIP_LOCAL + (name_off[i + 1] - name_off[i]) + (b == ZH_ZIP_EMPTY ? 0u : (uint32_t)(file_off[b + 1] - file_off[b]));
      }
   part[tid] = sum;
   zh_sync();
   for (uint32_t d = 1; d < ZH_ZIP_SCAN_THREADS; d <<= 1) {   // inclusive scan of the chunks' sums
      const uint64_t v = tid >= d ? part[tid - d] : 0;
      zh_sync();
      part[tid] += v;
      zh_sync();
   }
   const uint64_t local_total = part[ZH_ZIP_SCAN_THREADS - 1];
   // (the central offsets need no scan of their own: a central record is 46 + name_len bytes, so record i starts at 46 * i + name_off[i] - name_off[0])
   const uint64_t central_total = (uint64_t)ZH_ZIP_CENTRAL * n + (name_off[n] - name_off[0]);
   const uint32_t failed = !assembled ? 1u : base_off + local_total + central_total >= ZH_ZIP_LIMIT ? 2u : 0u;
   if (tid == 0) {
      report->local_bytes = local_total;
      report->central_bytes = central_total;
      report->failed = failed;
      report->pad = 0;
   }
   if (failed) return;
   uint64_t at = part[tid] - sum;
   for (uint32_t i = lo; i < hi; i++) {
      const uint32_t b = entry_block ? entry_block[i] : i;
      zh_zip_entry_t e;
      e.local_off = base_off + at;
      e.name_len = name_off[i + 1] - name_off[i];
      e.comp_size = b == ZH_ZIP_EMPTY ? 0u : (uint32_t)(file_off[b + 1] - file_off[b]);
      e.size = b == ZH_ZIP_EMPTY ? 0u : blocks[b].n;
      e.crc32 = 0;   // (zh_zip_records': one workgroup is no place for a square-and-multiply per entry)
      entries[i] = e;
      src_off[i] = b == ZH_ZIP_EMPTY ? ~0ull : file_off[b];
      at += ZH_ZIP_LOCAL + e.name_len + e.comp_size;
   }
}

// One lane per entry, striding: its CRC-32 (zh_crc32_finish of the max-block's linear part; into the entry table as well, where only this kernel writes that field
// and zh_zip_copy does not read it), its local header and name in the local part, its central header and name in the central part (out + central_at). Single bytes of
// its own records only. Workgroups of up to ZH_ZIP_RECORD_THREADS lanes (the host may launch fewer).
#define ZH_ZIP_RECORD_THREADS 64
__global__ void __launch_bounds__(ZH_ZIP_RECORD_THREADS)
zh_zip_records(zh_zip_entry_t *entries, const uint64_t *__restrict__ src_off, const uint32_t *__restrict__ name_off, const uint8_t *__restrict__ names,
               const uint32_t *__restrict__ entry_block, const uint32_t *__restrict__ crc, uint32_t n, uint64_t base_off, uint32_t dos_datetime, uint64_t central_at, const zh_zip_report_t *__restrict__ report, uint8_t *out) {
   if (report->failed) return;
   for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
      zh_zip_entry_t e = entries[i];
      const bool empty = src_off[i] == ~0ull;
      e.crc32 = empty ? 0u : zh_crc32_finish(crc[entry_block ? entry_block[i] : i], e.size);
      entries[i].crc32 = e.crc32;
      const uint8_t *name = names + name_off[i];
      uint8_t *l = out + (e.local_off - base_off), *c = out + central_at + (uint64_t)ZH_ZIP_CENTRAL * i + (name_off[i] - name_off[0]);
      zh_put_le(l, 0x04034b50u, 4);
      zh_put_le(c, 0x02014b50u, 4);
      zh_put_le(c + 4, 20, 2);                          // version made by
      // from here the two records agree: version needed, flags (bit 11: the name is UTF-8), method, time, date, CRC-32, sizes, name length, extra length
      for (uint32_t k = 0; k < 2; k++) {
         uint8_t *p = k ? c + 6 : l + 4;
         zh_put_le(p, empty ? 10 : 20, 2);
         zh_put_le(p + 2, 0x0800, 2);
         zh_put_le(p + 4, empty ? 0 : 8, 2);
         zh_put_le(p + 6, dos_datetime, 4);             // time, date
         zh_put_le(p + 10, e.crc32, 4);
         zh_put_le(p + 14, e.comp_size, 4);
         zh_put_le(p + 18, e.size, 4);
         zh_put_le(p + 22, e.name_len, 2);
         zh_put_le(p + 24, 0, 2);
      }
      zh_put_le(c + 32, 0, 4);                          // comment length, disk
      zh_put_le(c + 36, 0, 2);                          // internal attributes
      zh_put_le(c + 38, 0, 4);                          // external attributes
      zh_put_le(c + 42, (uint32_t)e.local_off, 4);
      for (uint32_t k = 0; k < e.name_len; k++) l[ZH_ZIP_LOCAL + k] = c[ZH_ZIP_CENTRAL + k] = name[k];
   }
}

// The streams, from stream + src_off[e] to behind entry e's name. Source and destination are at byte addresses independent of each other; the interior of a stream — the
// 16-byte chunks of the DESTINATION that lie wholly inside it — goes out as one 16-byte store per chunk, the bytes in front of and behind the interior one by one.
// Work is (entry, slice): a wave takes an entry, of ZH_ZIP_COPY_THREADS / 64 per workgroup, and of that entry the slices y, y + yslices, ... of ZH_ZIP_SLICE_CHUNKS
// chunks, where workgroup g is x = g / yslices along the entries and y = g % yslices along the slices (a one-dimensional grid of a multiple of yslices workgroups:
// the host sizes yslices by the largest input of the batch, it needs no count from the device). An entry of 2 MiB is 256 slices.
#define ZH_ZIP_COPY_THREADS 256
#define ZH_ZIP_MAX_YSLICES 32u
__global__ void __launch_bounds__(ZH_ZIP_COPY_THREADS)
zh_zip_copy(const zh_zip_entry_t *__restrict__ entries, const uint64_t *__restrict__ src_off, uint32_t n, uint64_t base_off, uint32_t yslices, const uint8_t *__restrict__ stream,
            const zh_zip_report_t *__restrict__ report, uint8_t *out) {
   if (report->failed) return;
   const uint32_t lane = threadIdx.x & 63u, waves = blockDim.x >> 6;
   const uint32_t y = blockIdx.x % yslices, x = blockIdx.x / yslices, xdim = gridDim.x / yslices;
   const uint64_t mask = ~(uint64_t)15;
   for (uint32_t e = x * waves + (threadIdx.x >> 6); e < n; e += xdim * waves) {
      const uint64_t s0 = src_off[e];
      if (s0 == ~0ull) continue;
      const zh_zip_entry_t en = entries[e];
      const uint64_t d0 = en.local_off - base_off + ZH_ZIP_LOCAL + en.name_len, d1 = d0 + en.comp_size;
      const uint64_t a0 = min((d0 + 15) & mask, d1), a1 = max(d1 & mask, a0);   // the interior: [a0, a1), whole chunks; the edges [d0, a0) and [a1, d1), 15 bytes at most each
      const uint64_t delta = s0 - d0;                                               // destination byte d comes from source byte d + delta (modulo 2^64)
      if (y == 0 && lane < 32) {
         const uint64_t d = lane < 16 ? d0 + lane : a1 + (lane - 16);
         if (d < (lane < 16 ? a0 : d1)) out[d] = stream[d + delta];
      }
      // the interior (zh_copy.h). Its aligned loads may reach up to 15 bytes in front of the stream and up to 15 behind its end — inside the stream buffer, which
      // starts aligned and has 16 bytes of slack.
      zh_copy_chunks(out + a0, stream + (a0 + delta), (uint32_t)((a1 - a0) >> 4), y, yslices, lane);
   }
}
#endif
