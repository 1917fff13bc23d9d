// tests/emul/order_expect.h - what the ordering kernels (csrc/k_order.h) must leave for a read, computed on the host with the product's
// own statement: the read's records sorted by (subject, hit order, position in the binned segment), then mc_build_stacks (mc_finish.h).
// pool: the HSP records; slots[heads[r] .. heads[r + 1]): the pool slots of read r's segment, in binned order.
// vexp: as many records as slots (read r's stacks at heads[r]; the rest zero), vn[r]: the size of its stacks.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>
#include "mc_finish.h"

inline void order_expected(const McHsp *pool, const uint32_t *slots, const uint32_t *heads, uint32_t nreads, McHsp *vexp, uint32_t *vn)
{
    memset(vexp, 0, (size_t)heads[nreads] * sizeof(McHsp));
    std::vector<uint32_t> idx;
    std::vector<McHsp> in;
    for (uint32_t r = 0; r < nreads; r++) {
        const uint32_t a = heads[r], n = heads[r + 1] - a;
        vn[r] = 0;
        if (!n) continue;
        idx.resize(n);
        for (uint32_t k = 0; k < n; k++) idx[k] = k;
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) {
            const McHsp &p = pool[slots[a + x]], &q = pool[slots[a + y]];
            return p.sidx != q.sidx ? p.sidx < q.sidx : p.chrono < q.chrono;
        });
        in.resize(n);
        for (uint32_t k = 0; k < n; k++) in[k] = pool[slots[a + idx[k]]];
        vn[r] = (uint32_t)mc_build_stacks(in.data(), (int)n, vexp + a);
    }
}
