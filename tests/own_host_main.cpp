// The two owners of pg_own.hpp on the host (tests/test_own_host.py builds this with -fsanitize=address,undefined and runs it): pg_dev_alloc / pg_dev_free over malloc /
// free with a table of live blocks and a switch that makes the k-th allocation fail.  One scripted life of a handle -- five get, one adopt from a CallBufs, two drop,
// one replace -- runs once without a failure and once for every allocation of the script failing; after each run: no live block, no block freed twice, every member
// null, and a CallBufs that gave a buffer did not free it.
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include "pg_own.hpp"

static std::set<void*> g_live;
static int g_allocs = 0, g_fail_at = 0, g_bad_free = 0;      // g_fail_at: the allocation (1-based) that fails; 0: none

int pg_dev_alloc(void** p, size_t bytes) {
    if (++g_allocs == g_fail_at) return 2;                    // (an allocator's "out of memory": p is left alone)
    *p = malloc(bytes ? bytes : 1);
    g_live.insert(*p);
    return 0;
}
void pg_dev_free(void* p) {
    if (!p) return;
    if (g_live.erase(p) != 1) { g_bad_free++; return; }      // freed twice, or never allocated: counted, and kept from the real free
    free(p);
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "own_host_main: line %d: %s (failing allocation %d)\n", __LINE__, #cond, g_fail_at); exit(1); } } while (0)

// what a handle keeps: pointer members of several types, two of them inside a nested record, and the owner (here a reference: run() lets the members outlive the
// owner, so that they can be read after it has died)
struct Handle {
    double* a = nullptr; int* b = nullptr; char* c = nullptr;
    struct Lib { float* recs = nullptr; int* idx = nullptr; } lib;
    float* table = nullptr;
    HandleBufs& mem;
};

// one call that builds in its own buffers and hands one of them over: false = an allocation failed and the call returned early
static bool install(Handle& h, float*& member, size_t n) {
    CallBufs D; float *fresh = nullptr, *scratch = nullptr;
    if (D.alloc(scratch, 3 * n)) return false;
    if (D.alloc(fresh, n)) return false;
    fresh[0] = 1.0f; scratch[0] = 2.0f;
    float* const given = fresh;
    h.mem.adopt(member, D.give(fresh));
    CHECK(fresh == nullptr && member == given);
    return true;                                              // (D dies here: it frees scratch and must not free `given`)
}

// the script: returns at the first failed allocation, as an entry point does
static void script(Handle& h) {
    if (h.mem.get(h.a, 10)) return;
    if (h.mem.get(h.b, 20)) return;
    if (h.mem.get(h.c, 30)) return;
    if (h.mem.get(h.lib.recs, 4)) return;
    if (h.mem.get(h.lib.idx, 8)) return;
    { double* const was = h.a; CHECK(h.mem.get(h.a, 10) == 0 && h.a == was); }      // a member that has its buffer keeps it: no allocation
    h.a[9] = 1.0; h.b[19] = 2; h.c[29] = 3; h.lib.recs[3] = 4.0f; h.lib.idx[7] = 5;
    if (!install(h, h.table, 16)) return;                                           // adopt into an empty member
    CHECK(g_live.count(h.table) == 1 && h.table[0] == 1.0f);                        // the CallBufs that gave it is gone and did not free it
    h.mem.drop(h.b); h.mem.drop(h.lib.idx);                                         // two drops
    CHECK(h.b == nullptr && h.lib.idx == nullptr);
    h.mem.drop(h.b);                                                                // (a member without a buffer: nothing happens)
    float* const old = h.table;
    if (!install(h, h.table, 32)) { CHECK(h.table == old && g_live.count(old) == 1); return; }      // a failed replace leaves the old buffer in place
    CHECK(h.table != nullptr && g_live.count(h.table) == 1 && h.table[0] == 1.0f);  // replace: the old buffer was freed, the new one is the handle's
    if (h.mem.get(h.b, 5)) return;                                                  // get after drop
    h.b[4] = 6;
}

static int run(int fail_at) {
    g_allocs = 0; g_fail_at = fail_at; g_bad_free = 0;
    HandleBufs* const mem = new HandleBufs();
    Handle h{nullptr, nullptr, nullptr, {}, nullptr, *mem};
    script(h);
    delete mem;
    CHECK(g_live.empty());
    CHECK(g_bad_free == 0);
    CHECK(!h.a && !h.b && !h.c && !h.lib.recs && !h.lib.idx && !h.table);
    return g_allocs;
}

int main() {
    const int n = run(0);
    CHECK(n == 10);                                             // 5 get + 2 x (scratch, fresh) + 1 get
    for (int k = 1; k <= n; k++) { const int made = run(k); CHECK(made == k); }
    printf("own_host_main: %d allocations, %d runs: ok\n", n, n + 1);
    return 0;
}
