// Who frees device memory: the two owners of pg_api.hip.  Plain C++17 with no HIP include: pg_api.hip defines pg_dev_alloc / pg_dev_free as hipMalloc / hipFree (its only
// calls of either), tests/own_host_main.cpp as malloc / free with a live-block table, so the owners' logic runs on the host under sanitizers.
#pragma once
#include <stddef.h>
#include <string.h>
#include <vector>
int pg_dev_alloc(void** p, size_t bytes);      // 0, or the allocator's error code
void pg_dev_free(void* p);
// The device memory of one call: alloc() remembers what it allocated, and what the call still holds is freed on every way out.  give() is the one way a buffer leaves:
// to the handle (HandleBufs::adopt), which owns it from then on (the caller's pointer is nulled: nothing in the call reads the buffer afterwards)
struct CallBufs {
    std::vector<void*> held;
    CallBufs() = default; CallBufs(const CallBufs&) = delete; CallBufs& operator=(const CallBufs&) = delete;
    ~CallBufs() { for (void* p : held) if (p) pg_dev_free(p); }
    template <class T> int alloc(T*& p, size_t count) { p = nullptr; void* q = nullptr; const int e = pg_dev_alloc(&q, count * sizeof(T)); if (e == 0) { held.push_back(q); p = (T*)q; } return e; }
    template <class T> T* give(T*& p) { for (void*& q : held) if (q == (void*)p) q = nullptr; T* const out = p; p = nullptr; return out; }
};
// The device memory of the handle, the LAST member of pg_handle (it dies first, while the pointers it nulls are alive).  It records the ADDRESS of every pointer member
// that owns a buffer, not the buffer: whoever frees also nulls the member, in one place.  The handle is never copied or moved, so the addresses hold
struct HandleBufs {
    std::vector<void*> slots;
    HandleBufs() = default; HandleBufs(const HandleBufs&) = delete; HandleBufs& operator=(const HandleBufs&) = delete;
    ~HandleBufs() { for (void* s : slots) { void* b; memcpy(&b, s, sizeof b); pg_dev_free(b); memset(s, 0, sizeof b); } }      // (a member is some T*: read and nulled as bytes)
    // `count` elements for member p, unless it has its buffer already
    template <class T> int get(T*& p, size_t count) { if (p) return 0; void* q = nullptr; const int e = pg_dev_alloc(&q, count * sizeof(T)); if (e == 0) { slots.push_back(&p); p = (T*)q; } return e; }
    // member p takes `buffer`, which a CallBufs gave (nullptr: nothing to own); what p held before is freed
    template <class T> void adopt(T*& p, T* buffer) { drop(p); if (buffer) { slots.push_back(&p); p = buffer; } }
    // frees the buffer of member p, nulls p and forgets it
    template <class T> void drop(T*& p) {
        for (size_t i = 0; i < slots.size(); i++) if (slots[i] == (void*)&p) { pg_dev_free((void*)p); slots.erase(slots.begin() + (ptrdiff_t)i); break; }
        p = nullptr;
    }
};
