// TEST INFRASTRUCTURE ONLY: the drivers' device buffers (vcfc_dec::Buffers) as
// host memory, for the emu_*_api.cpp entry points.  A slot that grows is
// filled with 0xCD, so a driver that relies on a slot's earlier contents, or
// reads what no kernel wrote, gives wrong bytes and not stale right ones.
#pragma once
#include <sys/mman.h>
#include <unistd.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vcfc_decode_driver.h"

struct HostBuffers : vcfc_dec::Buffers {
    std::vector<uint8_t> b[N_SLOTS];   // exactly the bytes asked for (operator new aligns them to 16)
    void *get(int slot, uint64_t bytes) override {
        if (b[slot].size() < bytes) b[slot].assign(bytes, 0xCD);   // poison
        return b[slot].data();
    }
};

// The input [src, src + n) of an emulated device entry.  Below 2 GiB it is a
// copy: 64 bytes of 0xCD behind it, or (guard) a copy that ends at a page
// with no access, so that a read past the last record's end faults.  From
// 2 GiB up the caller's memory is used in place -- a copy would touch all of
// it --, and the caller guarantees 64 readable bytes behind it.
struct HostInput {
    static constexpr uint64_t IN_PLACE = 1ull << 31;
    std::vector<uint8_t> copy;
    uint8_t *map = nullptr;
    size_t len = 0;
    const uint8_t *p = nullptr;
    HostInput(const uint8_t *src, uint64_t n, bool guard = false) {
        if (n >= IN_PLACE) {
            p = src;
        } else if (!guard) {
            if (src) copy.assign(src, src + n);
            copy.resize(n + 64, 0xCD);
            p = copy.data();
        } else {
            const size_t pg = (size_t)sysconf(_SC_PAGESIZE);
            const size_t body = (n + pg - 1) / pg * pg;
            len = body + pg;
            map = static_cast<uint8_t *>(mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0));
            if (map == MAP_FAILED) abort();
            mprotect(map + body, pg, PROT_NONE);
            if (n) memcpy(map + body - n, src, n);
            p = map + body - n;
        }
    }
    ~HostInput() {
        if (map) munmap(map, len);
    }
    HostInput(const HostInput &) = delete;
    HostInput &operator=(const HostInput &) = delete;
};
