// line_index_probe.hip -- TEST INFRASTRUCTURE ONLY: the two phases of the line
// index (csrc/vcfc_ingest.hip) over a device buffer with every knob of
// vcfc_line_index in the caller's hand, all seven tables and the counts left
// in the caller's device arrays (tests/test_gpu_line_index.py).  Linked
// against libvcfc.so: the kernels that run are the product's own code
// objects.  The workspaces are the caller's too (sized with
// line_probe_layout), so it can poison them and read phase 2's line ends.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vcfc_device.h"

// out[0] = phase 1's workspace bytes for a chunk of n bytes, out[1] = phase
// 2's for n_lines lines, out[2] = where phase 2's workspace holds the line
// ends (n_lines x u64, in order)
extern "C" void line_probe_layout(uint64_t n, uint64_t n_lines, uint64_t *out) {
    const VcfcLineIndexLayout L = vcfc_line_index_layout(n, n_lines);
    out[0] = L.total1;
    out[1] = L.total2;
    out[2] = L.nl;
}

// Phase 1, the line count to the host, phase 2.  tab: seven device arrays in
// VcfcLineIndex's order (line_off, line_len, line_no, pass_off, pass_len,
// pass_no, pass_before), each with room for cap_lines entries; counts: 4 x
// u64 on the device; cands: host memory or null.  Returns 0, a HIP error + 100,
// or 1 / 2 when a workspace is too small, 3 when phase 1 counted more than
// cap_lines lines (nothing is placed then).
extern "C" int line_probe_index(const uint8_t *buf, uint64_t n, uint32_t S_hint, uint64_t hop_walkers, int learn,
                                uint32_t len_hint, const VcfcHopCands *cands, hipStream_t s, uint8_t *ws1,
                                uint64_t ws1_bytes, uint8_t *ws2, uint64_t ws2_bytes, uint64_t cap_lines, void **tab,
                                uint64_t *counts, uint64_t *lines_out) {
    const VcfcLineIndexLayout L1 = vcfc_line_index_layout(n, 0);
    if (L1.total1 > ws1_bytes) return 1;
    VcfcLineIndex x;
    x.line_off = static_cast<uint64_t *>(tab[0]);
    x.line_len = static_cast<uint32_t *>(tab[1]);
    x.line_no = static_cast<uint32_t *>(tab[2]);
    x.pass_off = static_cast<uint64_t *>(tab[3]);
    x.pass_len = static_cast<uint32_t *>(tab[4]);
    x.pass_no = static_cast<uint32_t *>(tab[5]);
    x.pass_before = static_cast<uint64_t *>(tab[6]);
    x.counts = counts;
    hipError_t e = vcfc_line_index(buf, n, ws1, L1, x, s, S_hint, hop_walkers, learn != 0, len_hint, cands);
    if (e != hipSuccess) return 100 + (int)e;
    uint64_t lines = 0;
    if ((e = hipMemcpyAsync(&lines, counts, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return 100 + (int)e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return 100 + (int)e;
    *lines_out = lines;
    if (lines > cap_lines) return 3;
    const VcfcLineIndexLayout L = vcfc_line_index_layout(n, lines);
    if (L.total2 > ws2_bytes) return 2;
    if ((e = vcfc_line_index_place(buf, n, lines, ws1, ws2, L, x, s)) != hipSuccess) return 100 + (int)e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return 100 + (int)e;
    return 0;
}
