// zh_host.h — what the host code of more than one source file needs (zh_device.hip, zh_inflate.hip, libzultra.cpp): nothing for a kernel in here.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#ifdef ZH_EMU
#include <mutex>
// the lock-step emulator (tests/emu) runs one kernel at a time on one OS thread's fibers: host threads that drive contexts of their
// own (libzultra.cpp: lanes of zultra_memory_compress) take turns here — one lock for the whole library, in however many files it is compiled. The product build has no such lock.
inline std::recursive_mutex g_emu_mutex;
#define ZH_EMU_SERIALIZE() std::lock_guard<std::recursive_mutex> emu_lock_(g_emu_mutex)
#else
#define ZH_EMU_SERIALIZE()
#endif

// (64-bit min / max by name: hipcc's host-side `min` picks the int overload for two 64-bit arguments — 0xFFFFFFFF became -1)
static inline uint64_t zh_min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
static inline uint64_t zh_max64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// Environment switches: part of the shipped library's surface
static inline int zh_env(const char *name, int dflt) {
   const char *e = getenv(name);
   return e ? atoi(e) : dflt;
}
static inline uint64_t zh_env64(const char *name, uint64_t dflt) {   // (a byte count)
   const char *e = getenv(name);
   return e ? (uint64_t)strtoull(e, NULL, 10) : dflt;
}

// Helpers one source file defines for another: declared here only, none of them leaves the shared object.
#define ZH_HIDDEN __attribute__((visibility("hidden")))
ZH_HIDDEN uint32_t zh_clamp_block(uint32_t n);                                                // zh_device.hip: a caller's max-block size as the library takes it (libzultra.c:87-92)
ZH_HIDDEN void zh_threaded_copy(uint8_t *dst, const uint8_t *src, size_t n, size_t piece);   // libzultra.cpp: a copy into pinned staging, over a few threads from 2 * piece bytes on
ZH_HIDDEN uint32_t zh_device_cus(int device);                                                 // zh_inflate.hip: compute units of a device (256 where it does not say)
extern "C" {
ZH_HIDDEN void *zh_device_upload(int device, const void *host, size_t n);                     // zh_inflate.hip, for libzultra.cpp (which has no HIP of its own): a device copy of a host buffer
ZH_HIDDEN void zh_device_release(void *p);
}
