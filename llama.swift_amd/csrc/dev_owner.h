// dev_owner.h -- the one owner of device memory: a registry of {pointer, bytes, kind} behind raw-pointer members.  No HIP header: the
// allocator is two function pointers (the library's defaults are in llamahip.cpp), so tools/host_sanitize drives it with stubs over malloc.
// The rule: whoever holds a DevOwner allocates through it and frees nothing by hand -- release() where a buffer is regrown
// or dropped, the destructor for everything else; a group of buffers that are used together is allocated by alloc_all, all or none.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <vector>

namespace lh {

enum { MEM_DEVICE = 0, MEM_MAILBOX = 1, MEM_PINNED = 2 };      // device; uncached / fine-grained device (pipeline mailboxes); pinned, device-mapped host
// 0 = success, else the runtime's error code (hipError_t in the library).  zero: the block is zero-filled before the call returns.
typedef int (*DevAllocFn)(void **p, size_t bytes, int kind, bool zero);
typedef void (*DevReleaseFn)(void *p, int kind);
int dev_alloc_default(void **p, size_t bytes, int kind, bool zero);      // llamahip.cpp
void dev_release_default(void *p, int kind);

struct DevOwner {
    struct Entry { void *p; size_t bytes; int kind; };
    struct Want {      // one buffer of a group
        void **slot; size_t bytes; bool zero; int kind;
        template <class T> Want(T **s, size_t b, bool z = false, int k = MEM_DEVICE) : slot((void **) s), bytes(b), zero(z), kind(k) {}
    };
    std::vector<Entry> entries;
    DevAllocFn alloc_fn;
    DevReleaseFn release_fn;
    // live registrations / bytes of every owner of the process (llamahip_debug_live_allocs: a leak shows as a count that does not come back)
    static inline std::atomic<int64_t> live_n{0}, live_bytes{0};

    explicit DevOwner(DevAllocFn a = dev_alloc_default, DevReleaseFn r = dev_release_default) : alloc_fn(a), release_fn(r) {}
    DevOwner(const DevOwner &) = delete;
    DevOwner &operator=(const DevOwner &) = delete;
    ~DevOwner() { while (!entries.empty()) drop(entries.size() - 1); }

    // every buffer of the group or none: on failure what was got is released, every slot is null and the error is returned
    int alloc_all(std::initializer_list<Want> group) {
        for (const Want &w : group) *w.slot = nullptr;
        entries.reserve(entries.size() + group.size());
        const size_t n0 = entries.size();
        for (const Want &w : group) {
            void *p = nullptr;
            const int e = alloc_fn(&p, w.bytes, w.kind, w.zero);
            if (e != 0 || !p) {
                while (entries.size() > n0) drop(entries.size() - 1);
                for (const Want &u : group) *u.slot = nullptr;
                return e != 0 ? e : 2;      // (2: out of memory, a null block reported as success)
            }
            entries.push_back({ p, w.bytes, w.kind });
            live_n++; live_bytes += (int64_t) w.bytes;
            *w.slot = p;
        }
        return 0;
    }
    template <class T> int alloc(T **slot, size_t count, bool zero = false, int kind = MEM_DEVICE) {
        return alloc_all({ Want(slot, count * sizeof(T), zero, kind) });
    }
    int alloc(void **slot, size_t bytes, bool zero = false, int kind = MEM_DEVICE) { return alloc_all({ Want(slot, bytes, zero, kind) }); }
    // frees, unregisters and nulls; a null slot is a no-op
    template <class T> void release(T **slot) {
        if (!*slot) return;
        for (size_t i = entries.size(); i-- > 0;)
            if (entries[i].p == (void *) *slot) { drop(i); break; }
        *slot = nullptr;
    }

private:
    void drop(size_t i) {
        const Entry en = entries[i];
        entries.erase(entries.begin() + (long) i);
        live_n--; live_bytes -= (int64_t) en.bytes;
        release_fn(en.p, en.kind);
    }
};

}  // namespace lh
