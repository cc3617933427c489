// TEST INFRASTRUCTURE ONLY: the drivers' device buffers (vcfc_dec::Buffers) as
// host memory, for the emu_*_api.cpp entry points.  A slot that grows is
// filled with 0xCD, so a driver that relies on a slot's earlier contents, or
// reads what no kernel wrote, gives wrong bytes and not stale right ones.
#pragma once
#include <cstdint>
#include <vector>

#include "vcfc_decode_driver.h"

struct HostBuffers : vcfc_dec::Buffers {
    std::vector<uint8_t> b[N_SLOTS];   // exactly the bytes asked for (operator new aligns them to 16)
    void *get(int slot, uint64_t bytes) override {
        if (b[slot].size() < bytes) b[slot].assign(bytes, 0xCD);   // poison
        return b[slot].data();
    }
};
