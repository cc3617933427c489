// TEST INFRASTRUCTURE ONLY: diagnostic hooks for the emulator build -- count
// the rows that take the general path (emu_api.cpp reads it).
#pragma once
#define VCFC_DIAG_ROW_BEGIN()
#define VCFC_DIAG_ROW_END(a, row)
#define VCFC_DIAG_GENERAL_ROW(a) \
    if (vw::lane_id() == 0) atomicAdd((a).retry_count, 1u)
#define VCFC_DIAG_WS_BYTES(n) 0ull
// bytes the hop line index's walkers load (k_nl_hop), summed per process
void emu_diag_hop_read(unsigned long long bytes);
#define VCFC_DIAG_HOP_READ(bytes) emu_diag_hop_read((unsigned long long)(bytes))
// the hop walkers' steps (k_nl_hop), counted per process by kind
enum EmuHopStep {
    HOPSTEP_LINE_FIRST, HOPSTEP_LINE_CHECK, HOPSTEP_VERIFY_HIT, HOPSTEP_VERIFY_MISS, HOPSTEP_FIND, HOPSTEP_TRY_HIT,
    HOPSTEP_TRY_MISS, HOPSTEP_LEARN, HOPSTEP_GUESS_TAKEN, HOPSTEP_GUESS_FAIL, HOPSTEP_TRUST_ZERO, HOPSTEP_N
};
void emu_diag_hop_step(int what);
#define VCFC_DIAG_HOP_STEP(what) emu_diag_hop_step(HOPSTEP_##what)
