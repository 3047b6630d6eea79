// host_util.h -- what the host translation units (llamahip.cpp, ops.cpp, quantize.cpp) share: the error text, HIP error handling, the
// host-built tables, and the owning scratch of a single-op call.  Host .cpp files only: no .hip kernel file includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/llamahip.h"
#include "dev_owner.h"

namespace lh {

void set_err(char *err, size_t cap, const char *fmt, ...) __attribute__((format(printf, 3, 4)));      // llamahip.cpp

#define HIP_TRY(expr, code)                                                                          \
    do {                                                                                             \
        hipError_t e_ = (hipError_t) (expr);      /* (DevOwner reports the runtime's codes as int) */ \
        if (e_ != hipSuccess) {                                                                      \
            lh::set_err(err, err_cap, "HIP error: %s (%s) at %s:%d", hipGetErrorString(e_), #expr, __FILE__, __LINE__); \
            return (code);                                                                           \
        }                                                                                            \
    } while (0)

// there is no CPU fallback: 0 with a device, else LLAMAHIP_ERR_PREDICT and the message
inline int need_device(char *err, size_t err_cap) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev >= 1) return 0;
    set_err(err, err_cap, "no HIP device available: libllamahip has no CPU fallback");
    return LLAMAHIP_ERR_PREDICT;
}

// the silu and exp tables of ggml_init (ggml.c:2376-2389) and the RoPE angle table [n_ctx][dh/2][cos, sin] (ggml.c:7113-7116), host libm
// (llamahip.cpp: a model load and llamahip_op_attention upload the same ones)
void lut_tables(std::vector<uint16_t> &ts, std::vector<uint16_t> &te);
std::vector<double> rope_table(int n_ctx, int dh);
// what llamahip_kv_shift_rows and llamahip_op_kv_shift refuse of a table of shifts (llamahip.cpp): 0 and `tab` filled, or LLAMAHIP_ERR_PREDICT and
// the message naming the limit; slots_of is appended to the slot-range message (what bounds the slots, or "")
struct KvShiftTab;
int kv_shift_table_check(int32_t n_slots, const char *slots_of, int32_t n_ctx, int32_t n_shifts, const int32_t *slot, const int32_t *row_begin, const int32_t *n_rows,
                         const int32_t *n_discard, KvShiftTab &tab, const char *fn, char *err, size_t err_cap);

// QA operand (kcommon.hip.h quantize_y: rows Kp / 4 dwords and Kp / 32 scales apart, Kp = K rounded up to 256; dword (c * 8 + k) * 8 + j
// of a row holds chain k of block c * 8 + j as signed nibbles, shifted 4 bits in odd blocks) -> N rows of K / 32 Q4_0 blocks in file
// layout: {d, qs[16]}, qs[k] = (q[2k] + 8) | (q[2k+1] + 8) << 4
inline void qa_to_q4_0_blocks(const uint32_t *qa_A, const float *qa_d, int N, int K, uint8_t *out) {
    const int Kp = (K + 255) / 256 * 256;
    for (int n = 0; n < N; n++)
        for (int b = 0; b < K / 32; b++) {
            const uint32_t *A = qa_A + (size_t) n * (Kp / 4);
            uint8_t *blk = out + ((size_t) n * (K / 32) + b) * 20;
            memcpy(blk, &qa_d[(size_t) n * (Kp / 32) + b], 4);
            const int c = b >> 3, j = b & 7;
            for (int k = 0; k < 8; k++) {
                const uint32_t w = A[(c * 8 + k) * 8 + j] >> (4 * (j & 1));
                const uint32_t q0 = (w & 0xF) ^ 8, q1 = ((w >> 8) & 0xF) ^ 8, q2 = ((w >> 16) & 0xF) ^ 8, q3 = ((w >> 24) & 0xF) ^ 8;
                blk[4 + k] = (uint8_t) (q0 | (q1 << 4));
                blk[12 + k] = (uint8_t) (q2 | (q3 << 4));
            }
        }
}

// The owning holders of what is not memory.  Events: created through it, destroyed with it.
struct Events {
    std::vector<hipEvent_t> evs;
    Events() = default;
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    ~Events() { for (hipEvent_t ev : evs) (void) hipEventDestroy(ev); }
    hipError_t create(hipEvent_t *out, unsigned flags = hipEventDefault) {
        *out = nullptr;
        const hipError_t e = hipEventCreateWithFlags(out, flags);
        if (e == hipSuccess) evs.push_back(*out);
        return e;
    }
    size_t size() const { return evs.size(); }
    hipEvent_t operator[](size_t i) const { return evs[i]; }
};
// Captured steps by key: the cache owns its hipGraphExec_t values (an entry without one, exec == nullptr, is a step that runs un-captured).
// Whoever erases or clears waits for the device first where a caller's stream may still run an exec.  Payload: what travels with an entry.
struct NoPayload {};
template <class Key, class Payload = NoPayload> struct GraphCache {
    struct Entry : Payload { hipGraphExec_t exec = nullptr; };
    std::map<Key, Entry> map;
    GraphCache() = default;
    GraphCache(const GraphCache &) = delete;
    GraphCache &operator=(const GraphCache &) = delete;
    GraphCache(GraphCache &&o) noexcept : map(std::move(o.map)) { o.map.clear(); }      // (std::vector<StageSlot>::resize)
    ~GraphCache() { clear(); }
    Entry *find(const Key &k) { auto it = map.find(k); return it == map.end() ? nullptr : &it->second; }
    Entry *put(const Key &k, hipGraphExec_t exec, const Payload &p = Payload()) {
        erase(k);
        Entry &e = map[k];
        (Payload &) e = p; e.exec = exec;
        return &e;
    }
    void erase(const Key &k) {
        auto it = map.find(k);
        if (it == map.end()) return;
        if (it->second.exec) (void) hipGraphExecDestroy(it->second.exec);
        map.erase(it);
    }
    void clear() {
        for (auto &kv : map) if (kv.second.exec) (void) hipGraphExecDestroy(kv.second.exec);
        map.clear();
    }
    size_t size() const { return map.size(); }
};

// Device memory, a stream and events that live for ONE call.  The first HIP error sticks: after it alloc returns null and upload /
// download / fill / sync do nothing, so a body reads top to bottom, guards its launches with `if (s.ok()) s.check(launch_...)` and
// asks once at the end.  The destructor releases everything on every return path.
struct Scratch {
    DevOwner bufs;
    Events events;
    hipStream_t st = nullptr;
    hipError_t e = hipSuccess;
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { if (st) (void) hipStreamDestroy(st); }
    bool ok() const { return e == hipSuccess; }
    hipError_t error() const { return e; }
    void check(hipError_t r) { if (ok()) e = r; }
    template <class T> T *alloc(size_t count, const T *init = nullptr) {      // init: uploaded at once
        T *p = nullptr;
        if (ok()) check((hipError_t) bufs.alloc(&p, count));
        if (!ok()) return nullptr;
        if (init) upload(p, init, count * sizeof(T));
        return p;
    }
    // without a stream the copies and fills below are the synchronous ones on the null stream
    hipStream_t stream() { if (ok() && !st) check(hipStreamCreate(&st)); return st; }
    hipEvent_t event() { hipEvent_t ev = nullptr; if (ok()) check(events.create(&ev)); return ev; }
    void upload(void *dst, const void *src, size_t bytes) { if (ok()) check(st ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); }
    void download(void *dst, const void *src, size_t bytes) { if (ok()) check(st ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); }
    void fill(void *dst, int byte, size_t bytes) { if (ok()) check(st ? hipMemsetAsync(dst, byte, bytes, st) : hipMemset(dst, byte, bytes)); }
    void sync() { if (ok() && st) check(hipStreamSynchronize(st)); }
    // the one exit of a body that failed: the message names the entry point; the runtime's sticky last error is cleared with it
    int fail(const char *fn, char *err, size_t err_cap) const {
        (void) hipGetLastError();
        set_err(err, err_cap, "HIP error in %s: %s", fn, hipGetErrorString(e));
        return LLAMAHIP_ERR_PREDICT;
    }
};

}  // namespace lh
