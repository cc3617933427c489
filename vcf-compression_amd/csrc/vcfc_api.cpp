// vcfc_api.cpp -- the C ABI (include/vcfc.h): contexts, device buffers and
// the host-side drivers that mirror the reference's compress() loop
// (src/compress.cpp:205-257) around the GPU encoder.
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <sys/uio.h>

#include "vcfc.h"
#include "vcfc_decode_driver.h"
#include "vcfc_device.h"
#include "vcfc_index_driver.h"
#include "vcfc_ingest_driver.h"
#include "vcfc_sparse_index_driver.h"
#include "vcfc_subset_driver.h"
#include "vcfc_extract_driver.h"
#include "vcfc_counts_driver.h"
#include "vcfc_ld_driver.h"
#include "vcfc_kin_driver.h"
#include "vcfc_matrix_driver.h"
#include "vcfc_regions_driver.h"

hipError_t vcfc_sparse_plan_launch(const uint8_t *recs, const uint64_t *rec_off, uint64_t n, uint64_t data_start,
                                   uint64_t *file_off, uint8_t *prefix, uint64_t *status, hipStream_t s);
hipError_t vcfc_synth_device(uint8_t *buf, const uint64_t *line_off, uint64_t n, const uint8_t *prefix,
                             const uint64_t *prefix_off, const float *row_af, uint32_t S, int law,
                             uint64_t seed, uint64_t row_base, hipStream_t s);

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap && p) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(bytes, 1 << 20);
        want = want + want / 8;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Pinned host memory (the ingest pipeline's staging slots).
struct HostBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap && p) return hipSuccess;
        const size_t want = std::max<size_t>(std::max<size_t>(bytes, 2 * cap), 4096);   // geometric growth
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

}  // namespace

struct vcfc_timer {
    std::vector<hipEvent_t> ev;   // 6 per timed call (vcfc_encode_device)
    size_t used = 0;
};

struct vcfc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuf in, off, len, out, rec, ws, err, aux, flag, qref;
    DevBuf ing_dev[vcfc_ing::Memory::N_DEV];
    HostBuf ing_host[vcfc_ing::Memory::N_HOST];
    HostBuf dec_host[vcfc_dec::Buffers::N_HOST];
    uint64_t ingest_chunk = 0;   // 0: default (128 MiB)
    int line_index = VCFC_LINE_INDEX_HOP;
    int defer_records = VCFC_DEFER_DEFAULT;   // vcfc_ctx_set_deferred_records (on by default)
    unsigned trace = 0;          // VCFC_TRACE_* flags
};

namespace {

// Read-only mapping of an input file.
struct MappedFile {
    int fd = -1;
    const uint8_t *p = nullptr;
    uint64_t n = 0;
    int open_ro(const char *path) {
        fd = open(path, O_RDONLY);
        if (fd < 0) return VCFC_E_IO;
        struct stat st;
        if (fstat(fd, &st) != 0) return VCFC_E_IO;
        n = (uint64_t)st.st_size;
        if (n) {
            void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) return VCFC_E_IO;
            madvise(m, n, MADV_SEQUENTIAL);
            p = static_cast<const uint8_t *>(m);
        }
        return VCFC_OK;
    }
    ~MappedFile() {
        if (p) munmap(const_cast<uint8_t *>(p), n);
        if (fd >= 0) close(fd);
    }
};

// Metadata + header lines of a .vcfc: vcfc_dec::parse_header.
int parse_vcfc_header(const uint8_t *in, uint64_t n, uint64_t *data_off, uint64_t *sample_count) {
    return vcfc_dec::parse_header(in, n, data_off, sample_count);
}

// Record starts by hopping the LEN headers (read_compressed_line_length_headers,
// src/compress.cpp:270-331; both headers must carry extension count 3,
// src/utils.hpp:198-206).  rec[i] = offset of record i from `base`, rec[n] = end
// of the last whole record -- also where a bad header stops the walk, so the
// records before it are all indexed.
int index_records(const uint8_t *base, uint64_t n, std::vector<uint64_t> &rec) {
    rec.clear();
    uint64_t ip = 0;
    while (n - ip >= 8) {
        const uint8_t *h = base + ip;
        if ((h[0] >> 6) != 3 || (h[4] >> 6) != 3) break;
        const uint32_t L = ((uint32_t)(h[0] & 0x3F) << 24) | ((uint32_t)h[1] << 16) | ((uint32_t)h[2] << 8) | h[3];
        if (L < 4 || n - ip - 8 < (uint64_t)L - 4) break;
        rec.push_back(ip);
        ip += 8 + (L - 4);
    }
    rec.push_back(ip);
    return ip == n ? VCFC_OK : VCFC_E_FORMAT;
}

int write_all_at(int fd, const void *p, uint64_t len, uint64_t off) {
    const uint8_t *b = static_cast<const uint8_t *>(p);
    while (len) {
        ssize_t k = pwrite(fd, b, std::min<uint64_t>(len, 1ull << 30), (off_t)off);
        if (k <= 0) return VCFC_E_IO;
        b += k; len -= (uint64_t)k; off += (uint64_t)k;
    }
    return VCFC_OK;
}

// The sinks (vcfc_dec::Sink) of the calls that decode.  A buffer call's: counts
// every byte, copies while they fit (pass std::ref; VCFC_E_NOSPACE if !fits).
struct BufferSink {
    uint8_t *out;
    uint64_t cap, o = 0;
    bool fits = true;
    bool operator()(const uint8_t *p, uint64_t k) {
        if (fits && o + k <= cap) memcpy(out + o, p, k);
        else fits = false;
        o += k;
        return true;
    }
};
// of a call that writes to a descriptor the caller opened
struct FdSink {
    int fd;
    bool operator()(const uint8_t *p, uint64_t k) const {
        while (k) {
            const ssize_t w = write(fd, p, std::min<uint64_t>(k, 1ull << 30));
            if (w <= 0) return false;
            p += w;
            k -= (uint64_t)w;
        }
        return true;
    }
};
// of a call that writes a file of its own, at offsets from 0
struct FileSink {
    int fd;
    uint64_t o = 0;
    bool operator()(const uint8_t *p, uint64_t k) {
        if (write_all_at(fd, p, k, o)) return false;
        o += k;
        return true;
    }
};

void put_be64(uint8_t *o, uint64_t v) {
    for (int k = 0; k < 8; k++) o[k] = (uint8_t)(v >> (56 - 8 * k));
}

// The decoder's device buffers live in the context.
struct CtxDecodeBuffers : vcfc_dec::Buffers {
    vcfc_ctx *c;
    explicit CtxDecodeBuffers(vcfc_ctx *cc) : c(cc) {}
    void *get(int slot, uint64_t bytes) override {
        DevBuf *b = slot == IN ? &c->in : slot == REC ? &c->rec : slot == WS ? &c->ws : slot == OUT ? &c->out
                  : slot == LINE_OFF ? &c->off : slot == FLAG ? &c->flag
                  : slot == QREF ? &c->qref : &c->err;
        return b->ensure(bytes) == hipSuccess ? b->p : nullptr;
    }
    uint8_t *host(int slot, uint64_t bytes) override {   // pinned staging
        HostBuf &b = c->dec_host[slot];
        return b.ensure(bytes) == hipSuccess ? static_cast<uint8_t *>(b.p) : nullptr;
    }
};

// The ingest pipeline's buffers live in the context.
struct CtxIngestMemory : vcfc_ing::Memory {
    vcfc_ctx *c;
    explicit CtxIngestMemory(vcfc_ctx *cc) : c(cc) {}
    void *dev(int slot, uint64_t bytes) override {
        DevBuf &b = c->ing_dev[slot];
        return b.ensure(bytes) == hipSuccess ? b.p : nullptr;
    }
    void *host(int slot, uint64_t bytes) override {
        HostBuf &b = c->ing_host[slot];
        return b.ensure(bytes) == hipSuccess ? b.p : nullptr;
    }
};

// bytes [base, base + n) of a file
struct FdSource : vcfc_ing::Source {
    int fd;
    uint64_t n, base;
    FdSource(int f, uint64_t size, uint64_t base_off = 0) : fd(f), n(size), base(base_off) {}
    uint64_t size() const override { return n; }
    bool read(uint8_t *dst, uint64_t off, uint64_t k) override {
        off += base;
        while (k) {
            const ssize_t r = pread(fd, dst, std::min<uint64_t>(k, 1ull << 30), (off_t)off);
            if (r <= 0) return false;
            dst += r; off += (uint64_t)r; k -= (uint64_t)r;
        }
        return true;
    }
};

struct MemSource : vcfc_ing::Source {
    const uint8_t *p;
    uint64_t n;
    MemSource(const uint8_t *b, uint64_t size) : p(b), n(size) {}
    uint64_t size() const override { return n; }
    bool read(uint8_t *dst, uint64_t off, uint64_t k) override {
        memcpy(dst, p + off, k);
        return true;
    }
};

// chunk size: the context's (vcfc_ctx_set_ingest_chunk), else 128 MiB; never
// more than the input (rounded up to 4 KiB)
vcfc_ing::Config ingest_config(const vcfc_ctx *c, uint64_t n) {
    vcfc_ing::Config cfg;
    const uint64_t want = c->ingest_chunk ? c->ingest_chunk : (128ull << 20);
    cfg.chunk = std::min<uint64_t>(want, std::max<uint64_t>((n + 4095) & ~4095ull, 4096));
    cfg.trace = (c->trace & VCFC_TRACE_INGEST) != 0;
    cfg.defer_records = c->defer_records != 0;
    return cfg;
}

}  // namespace

extern "C" {

const char *vcfc_version(void) { return "vcfc-mi355x 0.1 (gfx950)"; }

const char *vcfc_strerror(int s) {
    switch (s) {
    case VCFC_OK: return "ok";
    case VCFC_E_LT8COLS: return "VCF data line did not contain at least 8 terms";
    case VCFC_E_8COLS: return "VCF data line has exactly 8 terms (reference aborts: std::length_error)";
    case VCFC_E_HEADER: return "VCF Header did not have enough columns";
    case VCFC_E_NOSPACE: return "output buffer too small";
    case VCFC_E_ARG: return "invalid argument";
    case VCFC_E_HIP: return "HIP runtime error (is a gfx950 GPU visible?)";
    case VCFC_E_IO: return "file I/O error";
    case VCFC_E_FORMAT: return "malformed .vcfc input";
    case VCFC_E_TOOLONG: return "VCF data line too long (its record could pass the 30-bit length header)";
    default: return "unknown status";
    }
}

int vcfc_ctx_create(int device, vcfc_ctx **out) {
    if (!out) return VCFC_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return VCFC_E_HIP;
    if (hipSetDevice(device) != hipSuccess) return VCFC_E_HIP;
    vcfc_ctx *c = new vcfc_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return VCFC_E_HIP;
    }
    *out = c;
    return VCFC_OK;
}

void vcfc_ctx_destroy(vcfc_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    c->in.release(); c->off.release(); c->len.release(); c->out.release();
    c->rec.release(); c->ws.release(); c->err.release(); c->aux.release();
    c->flag.release(); c->qref.release();
    for (auto &b : c->ing_dev) b.release();
    for (auto &b : c->ing_host) b.release();
    for (auto &b : c->dec_host) b.release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int vcfc_ctx_set_ingest_chunk(vcfc_ctx *c, uint64_t chunk_bytes) {
    if (!c || (chunk_bytes && (chunk_bytes < 4096 || chunk_bytes > (3ull << 30)))) return VCFC_E_ARG;
    c->ingest_chunk = chunk_bytes;
    return VCFC_OK;
}

int vcfc_ctx_set_line_index(vcfc_ctx *c, int mode) {
    if (!c || (mode != VCFC_LINE_INDEX_HOP && mode != VCFC_LINE_INDEX_SCAN)) return VCFC_E_ARG;
    c->line_index = mode;
    return VCFC_OK;
}

int vcfc_ctx_set_deferred_records(vcfc_ctx *c, int on) {
    if (!c || (on != 0 && on != 1)) return VCFC_E_ARG;
    c->defer_records = on;
    return VCFC_OK;
}

int vcfc_ctx_set_trace(vcfc_ctx *c, unsigned flags) {
    if (!c || (flags & ~(VCFC_TRACE_INGEST | VCFC_TRACE_DEVICE | VCFC_TRACE_SPARSE_QUERY | VCFC_TRACE_INDEX))) return VCFC_E_ARG;
    c->trace = flags;
    return VCFC_OK;
}

uint64_t vcfc_encode_bound(uint64_t n_rows, uint64_t total_line_bytes) {
    return vcfc_record_bound(n_rows, total_line_bytes);
}

uint64_t vcfc_encode_workspace_size(uint64_t n_rows, uint64_t total_line_bytes) {
    return vcfc_encode_workspace_layout(n_rows, total_line_bytes).total;
}

static int encode_rows_device_impl(const uint8_t *d_buf, const uint64_t *d_line_off, const uint32_t *d_line_len,
                                   uint64_t n, uint64_t total_line_bytes, uint8_t *d_out, uint64_t out_cap,
                                   uint64_t *d_rec_off, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream,
                                   hipEvent_t *ev) {
    if ((n && (!d_buf || !d_line_off || !d_line_len || !d_out)) || !d_rec_off || !d_err || (n && !d_ws))
        return VCFC_E_ARG;
    const VcfcWorkspaceLayout L = vcfc_encode_workspace_layout(n, total_line_bytes);
    if (ws_bytes < L.total) return VCFC_E_NOSPACE;
    uint8_t *ws = static_cast<uint8_t *>(d_ws);
    VcfcEncodeArgs a;
    a.buf = d_buf;
    a.line_off = d_line_off;
    a.line_len = d_line_len;
    a.n = n;
    a.line_bytes_hint = total_line_bytes;
    a.out = d_out;
    a.out_cap = out_cap;
    a.rec_off = d_rec_off;
    vcfc_encode_args_workspace(a, ws, L);
    a.err = d_err;
    return vcfc_encode_device(a, static_cast<hipStream_t>(stream), ev) == hipSuccess ? VCFC_OK : VCFC_E_HIP;
}

int vcfc_encode_rows_device(const uint8_t *d_buf, const uint64_t *d_line_off, const uint32_t *d_line_len,
                            uint64_t n, uint64_t total_line_bytes, uint8_t *d_out, uint64_t out_cap,
                            uint64_t *d_rec_off, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream) {
    return encode_rows_device_impl(d_buf, d_line_off, d_line_len, n, total_line_bytes, d_out, out_cap, d_rec_off,
                                   d_ws, ws_bytes, d_err, stream, nullptr);
}

int vcfc_encode_deferred_rows(const void *d_ws, uint64_t n, uint64_t total_line_bytes, void *stream,
                              uint64_t *rows) {
    if (!rows || (n && !d_ws)) return VCFC_E_ARG;
    *rows = 0;
    if (n == 0) return VCFC_OK;
    const VcfcWorkspaceLayout L = vcfc_encode_workspace_layout(n, total_line_bytes);
    uint32_t v = 0, fb = 0;   // deferred by k_encode_var, of which taken by the general path after all
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t *ws = static_cast<const uint8_t *>(d_ws);
    if (hipMemcpyAsync(&v, ws + vcfc_defer_count_offset(L), 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(&fb, ws + vcfc_defer_fallback_offset(L), 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return VCFC_E_HIP;
    *rows = v - fb;
    return VCFC_OK;
}

int vcfc_timer_create(vcfc_timer **t) {
    if (!t) return VCFC_E_ARG;
    *t = new vcfc_timer();
    return VCFC_OK;
}

void vcfc_timer_destroy(vcfc_timer *t) {
    if (!t) return;
    for (auto &e : t->ev) (void)hipEventDestroy(e);
    delete t;
}

int vcfc_encode_rows_device_timed(const uint8_t *d_buf, const uint64_t *d_line_off, const uint32_t *d_line_len,
                                  uint64_t n, uint64_t total_line_bytes, uint8_t *d_out, uint64_t out_cap,
                                  uint64_t *d_rec_off, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream,
                                  vcfc_timer *t) {
    if (!t) return VCFC_E_ARG;
    const size_t base = 6 * t->used;
    while (t->ev.size() < base + 6) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return VCFC_E_HIP;
        t->ev.push_back(e);
    }
    int st = encode_rows_device_impl(d_buf, d_line_off, d_line_len, n, total_line_bytes, d_out, out_cap, d_rec_off,
                                     d_ws, ws_bytes, d_err, stream, t->ev.data() + base);
    if (st == VCFC_OK) t->used++;
    return st;
}

int vcfc_timer_read(vcfc_timer *t, double ms[4], uint64_t *calls) {
    if (!t || !ms) return VCFC_E_ARG;
    for (int k = 0; k < 4; k++) ms[k] = 0;
    for (size_t i = 0; i < t->used; i++) {
        hipEvent_t *e = t->ev.data() + 6 * i;
        if (hipEventSynchronize(e[5]) != hipSuccess) return VCFC_E_HIP;
        for (int k = 0; k < 5; k++) {
            float f = 0;
            if (hipEventElapsedTime(&f, e[k], e[k + 1]) != hipSuccess) return VCFC_E_HIP;
            ms[k == 4 ? 1 : k] += f;   // k_encode_defer's deferred records count as k_encode
        }
    }
    if (calls) *calls = t->used;
    t->used = 0;
    return VCFC_OK;
}

int vcfc_synth_rows_device_at(uint8_t *d_buf, const uint64_t *d_line_off, uint64_t n, const uint8_t *d_prefix,
                              const uint64_t *d_prefix_off, const float *d_row_af, uint32_t samples, int law,
                              uint64_t seed, uint64_t row_base, void *stream) {
    if (n && (!d_buf || !d_line_off || !d_prefix || !d_prefix_off)) return VCFC_E_ARG;
    if (law < 0 || law > 3 || (law >= 2 && n && !d_row_af)) return VCFC_E_ARG;
    return vcfc_synth_device(d_buf, d_line_off, n, d_prefix, d_prefix_off, d_row_af, samples, law, seed, row_base,
                             static_cast<hipStream_t>(stream)) == hipSuccess
               ? VCFC_OK
               : VCFC_E_HIP;
}

int vcfc_synth_rows_device(uint8_t *d_buf, const uint64_t *d_line_off, uint64_t n, const uint8_t *d_prefix,
                           const uint64_t *d_prefix_off, const float *d_row_af, uint32_t samples, int law,
                           uint64_t seed, void *stream) {
    return vcfc_synth_rows_device_at(d_buf, d_line_off, n, d_prefix, d_prefix_off, d_row_af, samples, law, seed, 0,
                                     stream);
}

// Host batch: copy in, encode, copy out.  Synchronous on the context stream.
int vcfc_encode_rows(vcfc_ctx *c, const uint8_t *buf, uint64_t buf_bytes, const uint64_t *line_off,
                     const uint32_t *line_len, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *rec_off,
                     int64_t *err_row) {
    if (!c || !rec_off || (n && (!buf || !line_off || !line_len || !out))) return VCFC_E_ARG;
    if (err_row) *err_row = -1;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (line_off[i] + line_len[i] > buf_bytes) return VCFC_E_ARG;
        total += line_len[i];
    }
    const uint64_t bound = vcfc_encode_bound(n, total);
    const uint64_t wsz = vcfc_encode_workspace_size(n, total);
    if (c->in.ensure(buf_bytes + 64) || c->off.ensure(8 * n + 8) || c->len.ensure(4 * n + 8) ||
        c->out.ensure(bound) || c->rec.ensure(8 * (n + 1)) || c->ws.ensure(wsz) || c->err.ensure(8))
        return VCFC_E_HIP;
    hipStream_t s = c->stream;
    if (hipMemcpyAsync(c->in.p, buf, buf_bytes, hipMemcpyHostToDevice, s) ||
        hipMemcpyAsync(c->off.p, line_off, 8 * n, hipMemcpyHostToDevice, s) ||
        hipMemcpyAsync(c->len.p, line_len, 4 * n, hipMemcpyHostToDevice, s))
        return VCFC_E_HIP;
    int st = vcfc_encode_rows_device(static_cast<uint8_t *>(c->in.p), static_cast<uint64_t *>(c->off.p),
                                     static_cast<uint32_t *>(c->len.p), n, total, static_cast<uint8_t *>(c->out.p),
                                     c->out.cap, static_cast<uint64_t *>(c->rec.p), c->ws.p, c->ws.cap,
                                     static_cast<uint64_t *>(c->err.p), s);
    if (st != VCFC_OK) return st;
    uint64_t errw = 0;
    if (hipMemcpyAsync(rec_off, c->rec.p, 8 * (n + 1), hipMemcpyDeviceToHost, s) ||
        hipMemcpyAsync(&errw, c->err.p, 8, hipMemcpyDeviceToHost, s) || hipStreamSynchronize(s))
        return VCFC_E_HIP;
    uint64_t upto = n, status = VCFC_OK;
    if (errw != VCFCD_NO_ERROR) {
        upto = errw >> 8;
        status = errw & 0xFF;
        if (err_row) *err_row = (int64_t)upto;
    }
    const uint64_t bytes = rec_off[upto];
    if (bytes > out_cap) return VCFC_E_NOSPACE;
    if (bytes && (hipMemcpyAsync(out, c->out.p, bytes, hipMemcpyDeviceToHost, s) || hipStreamSynchronize(s)))
        return VCFC_E_HIP;
    return (int)status;
}

int vcfc_compress_data_line(vcfc_ctx *c, const char *line, uint64_t len, int add_newline, uint8_t *out,
                            uint64_t out_cap, uint64_t *out_len) {
    if (!c || !line || !out || !out_len || len > 0xFFFFFFFFull) return VCFC_E_ARG;
    const uint64_t off = 0;
    const uint32_t l32 = (uint32_t)len;
    uint64_t ro[2] = {0, 0};
    std::vector<uint8_t> tmp(vcfc_encode_bound(1, len) + 16);
    int64_t er = -1;
    int st = vcfc_encode_rows(c, reinterpret_cast<const uint8_t *>(line), len, &off, &l32, 1, tmp.data(),
                              tmp.size(), ro, &er);
    if (st != VCFC_OK) return st;
    uint64_t n = ro[1];
    if (!add_newline) n -= 1;  // records always end in '\n' (compress.cpp:188-190)
    if (n > out_cap) return VCFC_E_NOSPACE;
    if (!add_newline) {
        // LEN counts the record without the newline
        const uint32_t L = (uint32_t)(n - 4);
        tmp[0] = (uint8_t)(((L >> 24) & 0xFF) | 0xC0);
        tmp[1] = (uint8_t)((L >> 16) & 0xFF);
        tmp[2] = (uint8_t)((L >> 8) & 0xFF);
        tmp[3] = (uint8_t)(L & 0xFF);
    }
    memcpy(out, tmp.data(), n);
    *out_len = n;
    return VCFC_OK;
}

uint64_t vcfc_sparse_offset(uint64_t pos) { return (300000000ull + pos) * (4ull * 4096ull); }

int vcfc_sparse_plan_device(const uint8_t *d_recs, const uint64_t *d_rec_off, uint64_t n, uint64_t data_start,
                            uint64_t *d_file_off, uint8_t *d_prefix16, uint64_t *d_status, void *stream) {
    if ((n && (!d_recs || !d_rec_off || !d_file_off || !d_prefix16)) || !d_status) return VCFC_E_ARG;
    return vcfc_sparse_plan_launch(d_recs, d_rec_off, n, data_start, d_file_off, d_prefix16, d_status,
                                   static_cast<hipStream_t>(stream)) == hipSuccess
               ? VCFC_OK
               : VCFC_E_HIP;
}

// sparsify_file (reference src/sparse.cpp:290-580).  The GPU plans offsets
// and prefixes; the host writes one pwritev per record (the reference writes
// one byte per syscall) or, if the plan flags overlapping/out-of-order
// records, replays the reference's write sequence so later writes win as
// they do there.
namespace {

// Plan records [a, b) of the index on the GPU (k_sparse_plan): file offsets,
// 16-byte prefixes; status[0] = ~0 or (first unparsable record, local to a)
// << 8 | code, status[1] = 1 if adjacent records overlap or are out of order.
int sparse_plan_range(vcfc_ctx *c, const uint8_t *recs, const std::vector<uint64_t> &rec, uint64_t a, uint64_t b,
                      uint64_t data_start, std::vector<uint64_t> &file_off, std::vector<uint8_t> &prefix,
                      uint64_t status[2]) {
    const uint64_t n = b - a;
    file_off.assign(n, 0);
    prefix.assign(16 * n, 0);
    status[0] = ~0ull;
    status[1] = 0;
    if (!n) return VCFC_OK;
    const uint64_t base = rec[a], span = rec[b] - base;
    std::vector<uint64_t> ro(n + 1);
    for (uint64_t i = 0; i <= n; i++) ro[i] = rec[a + i] - base;
    if (c->in.ensure(span + 64) || c->rec.ensure(8 * (n + 1)) || c->out.ensure(16 * n) || c->off.ensure(8 * n) ||
        c->err.ensure(16))
        return VCFC_E_HIP;
    hipStream_t s = c->stream;
    if (hipMemcpyAsync(c->in.p, recs + base, span, hipMemcpyHostToDevice, s) ||
        hipMemcpyAsync(c->rec.p, ro.data(), 8 * (n + 1), hipMemcpyHostToDevice, s))
        return VCFC_E_HIP;
    if (vcfc_sparse_plan_launch(static_cast<uint8_t *>(c->in.p), static_cast<uint64_t *>(c->rec.p), n, data_start,
                                static_cast<uint64_t *>(c->off.p), static_cast<uint8_t *>(c->out.p),
                                static_cast<uint64_t *>(c->err.p), s) != hipSuccess)
        return VCFC_E_HIP;
    if (hipMemcpyAsync(file_off.data(), c->off.p, 8 * n, hipMemcpyDeviceToHost, s) ||
        hipMemcpyAsync(prefix.data(), c->out.p, 16 * n, hipMemcpyDeviceToHost, s) ||
        hipMemcpyAsync(status, c->err.p, 16, hipMemcpyDeviceToHost, s) || hipStreamSynchronize(s))
        return VCFC_E_HIP;
    return VCFC_OK;
}

// Write records g0 .. g0 + cnt - 1 (global indices; file_off / prefix point at
// record g0's plan) with one pwritev each; record 0 also fills the
// first-offset slot (host byte order, sparse.cpp:495-511).  replay (g0 == 0
// only): the reference's exact write sequence -- a record's dist_to_next goes
// out as 0 and the next record's step patches it (sparse.cpp:529-553) -- so
// later writes win where records overlap.
int sparse_write_range(int fd, const uint8_t *recs, const std::vector<uint64_t> &rec, uint64_t g0, uint64_t cnt,
                       const uint64_t *file_off, const uint8_t *prefix, uint64_t data_start, bool replay) {
    int w = VCFC_OK;
    for (uint64_t i = 0; i < cnt && !w; i++) {
        const uint64_t g = g0 + i;
        uint8_t pfx[16];
        memcpy(pfx, prefix + 16 * i, 16);
        if (g == 0) {
            const uint64_t voff = file_off[i] - data_start;
            w = write_all_at(fd, &voff, 8, data_start - 8);
        } else if (replay) {
            uint8_t d[8];
            put_be64(d, file_off[i] - file_off[i - 1]);
            w = write_all_at(fd, d, 8, file_off[i - 1] + 8);
        }
        if (w) break;
        if (replay) memset(pfx + 8, 0, 8);
        struct iovec iov[2] = {{pfx, 16}, {const_cast<uint8_t *>(recs + rec[g]), (size_t)(rec[g + 1] - rec[g])}};
        const uint64_t want = 16 + rec[g + 1] - rec[g];
        ssize_t k = pwritev(fd, iov, 2, (off_t)file_off[i]);
        if (k != (ssize_t)want) {
            // short write: finish the record plainly
            std::vector<uint8_t> tmp(want);
            memcpy(tmp.data(), pfx, 16);
            memcpy(tmp.data() + 16, recs + rec[g], want - 16);
            w = write_all_at(fd, tmp.data(), want, file_off[i]);
        }
    }
    return w;
}

// The .vcfc mapped, its header parsed and its records indexed.
struct SparseInput {
    MappedFile f;
    uint64_t data_in = 0, n = 0, data_start = 0;
    const uint8_t *recs = nullptr;
    std::vector<uint64_t> rec;
    int ist = VCFC_OK;   // index_records status (an error after the good prefix)
    int open(const char *path) {
        int st = f.open_ro(path);
        if (st) return st;
        if ((st = parse_vcfc_header(f.p, f.n, &data_in, nullptr))) return st;
        recs = f.p + data_in;
        ist = index_records(recs, f.n - data_in, rec);
        n = rec.size() - 1;
        data_start = data_in + 8;   // header lines + 8-byte slot
        return VCFC_OK;
    }
};

}  // namespace

int vcfc_sparsify_file(vcfc_ctx *c, const char *in_path, const char *out_path) {
    if (!c || !in_path || !out_path) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    SparseInput in;
    int st = in.open(in_path);
    if (st) {
        // the reference creates the output once the input is open and throws on
        // a bad header before it writes a byte: the output is left empty
        if (in.f.fd >= 0) {
            const int fd = open(out_path, O_CREAT | O_TRUNC | O_RDWR, 0600);
            if (fd >= 0) close(fd);
        }
        return st;
    }
    const uint64_t n = in.n;
    std::vector<uint64_t> file_off;
    std::vector<uint8_t> prefix;
    uint64_t status[2];
    if ((st = sparse_plan_range(c, in.recs, in.rec, 0, n, in.data_start, file_off, prefix, status))) return st;
    uint64_t upto = n;   // records before the first unparsable one are written
    if (status[0] != ~0ull && n) upto = status[0] >> 8;
    int fd = open(out_path, O_CREAT | O_TRUNC | O_RDWR, 0600);
    if (fd < 0) return VCFC_E_IO;
    int w = write_all_at(fd, in.f.p, in.data_in, 0);
    const uint8_t zero8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!w) w = write_all_at(fd, zero8, 8, in.data_in);
    if (!w)
        w = sparse_write_range(fd, in.recs, in.rec, 0, upto, file_off.data(), prefix.data(), in.data_start,
                               status[1] != 0);
    close(fd);
    if (w) return w;
    if (upto < n) return VCFC_E_FORMAT;
    return in.ist;
}

int vcfc_sparsify_shard(vcfc_ctx *c, const char *in_path, const char *out_path, int rank, int world,
                        uint64_t info[4]) {
    if (!c || !in_path || !info || world < 1 || rank < 0 || rank >= world) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    SparseInput in;
    int st = in.open(in_path);
    if (st) return st;
    const uint64_t n = in.n;
    const uint64_t lo = (uint64_t)((unsigned __int128)n * (unsigned)rank / (unsigned)world);
    const uint64_t hi = (uint64_t)((unsigned __int128)n * (unsigned)(rank + 1) / (unsigned)world);
    const uint64_t a = lo ? lo - 1 : 0, b = hi < n ? hi + 1 : n;   // one halo record each side
    std::vector<uint64_t> file_off;
    std::vector<uint8_t> prefix;
    uint64_t status[2] = {~0ull, 0};
    if (hi > lo && (st = sparse_plan_range(c, in.recs, in.rec, a, b, in.data_start, file_off, prefix, status)))
        return st;
    info[0] = lo;
    info[1] = hi;
    info[2] = status[0] != ~0ull ? a + (status[0] >> 8) : (in.ist ? n : ~0ull);
    info[3] = status[1];
    if (!out_path) return VCFC_OK;
    if (info[2] != ~0ull || info[3]) return VCFC_E_ARG;
    int fd = open(out_path, O_CREAT | O_WRONLY, 0600);
    if (fd < 0) return VCFC_E_IO;
    int w = VCFC_OK;
    if (rank == 0) {
        w = write_all_at(fd, in.f.p, in.data_in, 0);
        const uint8_t zero8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (!w && n == 0) w = write_all_at(fd, zero8, 8, in.data_in);   // else record 0's owner fills it
    }
    if (!w && hi > lo)
        w = sparse_write_range(fd, in.recs, in.rec, lo, hi - lo, file_off.data() + (lo - a),
                               prefix.data() + 16 * (lo - a), in.data_start, false);
    close(fd);
    return w;
}

uint64_t vcfc_compress_bound(uint64_t in_bytes) { return in_bytes + in_bytes / 2 + 64; }

// compress() (reference src/compress.cpp:205-257) through the pipelined
// ingest (csrc/vcfc_ingest_driver.h: reader threads -> GPU line index +
// encode -> writer thread).
int vcfc_compress_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t out_cap,
                         uint64_t *out_len, int64_t *err_line) {
    if (!c || (!in && n) || !out || !out_len) return VCFC_E_ARG;
    if (err_line) *err_line = -1;
    *out_len = 0;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    uint64_t o = 0;
    bool full = false;
    auto sink = [&](const uint8_t *p, uint64_t k) {
        if (o + k > out_cap) { full = true; return false; }
        memcpy(out + o, p, k);
        o += k;
        return true;
    };
    MemSource src(in, n);
    CtxIngestMemory M(c);
    const vcfc_ing::Config cfg = ingest_config(c, n);
    const int st = vcfc_ing::compress_stream(src, sink, M, c->stream, cfg, err_line);
    *out_len = o;
    if (full) return VCFC_E_NOSPACE;
    return st;
}

// compress() over VCF file bytes resident in device memory: line index +
// encoder on the GPU over the whole input at once (or chunks of the context's
// ingest chunk when one is set), output left in device memory
// (vcfc_ing::compress_device).
int vcfc_compress_device(vcfc_ctx *c, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t out_cap,
                         uint64_t *out_len, int64_t *err_line) {
    if (!c || (!d_in && n) || !d_out || !out_len) return VCFC_E_ARG;
    if (err_line) *err_line = -1;
    *out_len = 0;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    CtxIngestMemory M(c);
    vcfc_ing::Config cfg;
    cfg.max_chunk = 1ull << 40;   // (line lengths are 32-bit; the index's positions 64-bit)
    const uint64_t want = c->ingest_chunk ? c->ingest_chunk : cfg.max_chunk;
    cfg.chunk = std::min<uint64_t>(want, std::max<uint64_t>((n + 4095) & ~4095ull, 4096));
    cfg.hop_index = c->line_index == VCFC_LINE_INDEX_HOP;
    cfg.defer_records = c->defer_records != 0;
    cfg.trace = (c->trace & VCFC_TRACE_DEVICE) != 0;
    return vcfc_ing::compress_device(d_in, n, d_out, out_cap, out_len, M, c->stream, cfg, err_line);
}

int vcfc_compress_file(vcfc_ctx *c, const char *in_path, const char *out_path, int64_t *err_line) {
    if (!c || !in_path || !out_path) return VCFC_E_ARG;
    if (err_line) *err_line = -1;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    int fd = open(in_path, O_RDONLY);
    if (fd < 0) return VCFC_E_IO;
    struct stat st;
    if (fstat(fd, &st) != 0) { close(fd); return VCFC_E_IO; }
    const uint64_t n = (uint64_t)st.st_size;
    posix_fadvise(fd, 0, 0, POSIX_FADV_SEQUENTIAL);
    // the reference opens (truncates) the output before reading the input
    int ofd = open(out_path, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (ofd < 0) { close(fd); return VCFC_E_IO; }
    auto sink = [&](const uint8_t *p, uint64_t k) {
        while (k) {
            const ssize_t w = write(ofd, p, std::min<uint64_t>(k, 1ull << 30));
            if (w <= 0) return false;
            p += w;
            k -= (uint64_t)w;
        }
        return true;
    };
    FdSource src(fd, n);
    CtxIngestMemory M(c);
    const vcfc_ing::Config cfg = ingest_config(c, n);
    int s = vcfc_ing::compress_stream(src, sink, M, c->stream, cfg, err_line);
    close(fd);
    if (close(ofd) != 0 && s == VCFC_OK) s = VCFC_E_IO;
    return s;
}

// One rank's share of a sharded compress (SURVEY §8 e): the line-aligned byte
// range [off, off + len) of in_path through the same pipeline, its output
// written to out_fd from out_off on (pwrite; the caller places it).
int vcfc_compress_range(vcfc_ctx *c, const char *in_path, uint64_t off, uint64_t len, int out_fd, uint64_t out_off,
                        uint64_t *out_bytes, int64_t *err_line, uint64_t *lines) {
    if (!c || !in_path || out_fd < 0 || !out_bytes) return VCFC_E_ARG;
    *out_bytes = 0;
    if (err_line) *err_line = -1;
    if (lines) *lines = 0;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    int fd = open(in_path, O_RDONLY);
    if (fd < 0) return VCFC_E_IO;
    struct stat st;
    if (fstat(fd, &st) != 0 || off > (uint64_t)st.st_size || len > (uint64_t)st.st_size - off) {
        close(fd);
        return VCFC_E_ARG;
    }
    posix_fadvise(fd, (off_t)off, (off_t)len, POSIX_FADV_SEQUENTIAL);
    uint64_t o = 0;
    auto sink = [&](const uint8_t *p, uint64_t k) {
        if (write_all_at(out_fd, p, k, out_off + o)) return false;
        o += k;
        return true;
    };
    FdSource src(fd, len, off);
    CtxIngestMemory M(c);
    const vcfc_ing::Config cfg = ingest_config(c, len);
    const int s = vcfc_ing::compress_stream(src, sink, M, c->stream, cfg, err_line, lines);
    close(fd);
    *out_bytes = o;
    return s;
}

struct vcfc_held : vcfc_ing::Held {};

int vcfc_compress_range_held(vcfc_ctx *c, const char *in_path, uint64_t off, uint64_t len, uint64_t mem_bound,
                             const char *spill_dir, vcfc_held **held, uint64_t *out_bytes, int64_t *err_line,
                             uint64_t *lines) {
    if (!c || !in_path || !held || !out_bytes) return VCFC_E_ARG;
    *held = nullptr;
    *out_bytes = 0;
    if (err_line) *err_line = -1;
    if (lines) *lines = 0;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    int fd = open(in_path, O_RDONLY);
    if (fd < 0) return VCFC_E_IO;
    struct stat st;
    if (fstat(fd, &st) != 0 || off > (uint64_t)st.st_size || len > (uint64_t)st.st_size - off) {
        close(fd);
        return VCFC_E_ARG;
    }
    posix_fadvise(fd, (off_t)off, (off_t)len, POSIX_FADV_SEQUENTIAL);
    vcfc_held *h = new (std::nothrow) vcfc_held;
    if (!h) { close(fd); return VCFC_E_IO; }
    h->mem_bound = mem_bound;
    if (spill_dir) h->spill_dir = spill_dir;
    auto sink = [&](const uint8_t *p, uint64_t k) { return h->append(p, k); };
    FdSource src(fd, len, off);
    CtxIngestMemory M(c);
    const vcfc_ing::Config cfg = ingest_config(c, len);
    const int s = vcfc_ing::compress_stream(src, sink, M, c->stream, cfg, err_line, lines);
    close(fd);
    *held = h;
    *out_bytes = h->bytes();
    return s;
}

int vcfc_held_place(const vcfc_held *h, int out_fd, uint64_t out_off) {
    if (!h || out_fd < 0) return VCFC_E_ARG;
    return h->place(out_fd, out_off) ? VCFC_OK : VCFC_E_IO;
}

void vcfc_held_sizes(const vcfc_held *h, uint64_t *mem_bytes, uint64_t *spill_bytes) {
    if (mem_bytes) *mem_bytes = h ? h->mem : 0;
    if (spill_bytes) *spill_bytes = h ? h->spilled : 0;
}

void vcfc_held_free(vcfc_held *h) { delete h; }

// ---- decoder: decompress2_fd, reference
// src/compress.cpp:1214-1257 ------------------------------------------------

int vcfc_decompress_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t out_cap,
                           uint64_t *out_len) {
    if (!c || (!in && n) || (!out && out_cap) || !out_len) return VCFC_E_ARG;
    *out_len = 0;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    uint64_t data_off = 0, S = 0;
    int st = parse_vcfc_header(in, n, &data_off, &S);
    if (st) return st;   // the reference writes nothing before its header check passes
    BufferSink bs{out, out_cap};
    bs(in, data_off);
    CtxDecodeBuffers B(c);
    st = vcfc_dec::decode_section(in + data_off, n - data_off, S, B, c->stream, std::ref(bs));
    *out_len = bs.o;
    return bs.fits ? st : VCFC_E_NOSPACE;
}

int vcfc_decompress_file(vcfc_ctx *c, const char *in_path, const char *out_path) {
    if (!c || !in_path || !out_path) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    MappedFile f;
    int st = f.open_ro(in_path);
    if (st) return st;
    // the reference opens (truncates) the output before reading the headers
    int fd = open(out_path, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fd < 0) return VCFC_E_IO;
    uint64_t data_off = 0, S = 0;
    st = parse_vcfc_header(f.p, f.n, &data_off, &S);
    FileSink fs{fd};
    if (!st && !fs(f.p, data_off)) st = VCFC_E_IO;
    if (!st) {
        CtxDecodeBuffers B(c);
        st = vcfc_dec::decode_section(f.p + data_off, f.n - data_off, S, B, c->stream, std::ref(fs));
    }
    close(fd);
    return st;
}

// ---- range query: query_compressed_file, reference
// src/main.cpp:3777-3929 ----------------------------------------------------

// parse_coordinate_string (src/main.cpp:3993-4026): vcfc_regions_driver.h,
// where the region text parser shares it
int vcfc_parse_query(const char *q, uint64_t q_len, uint64_t *ref_len, int *has_range, uint64_t *start,
                     uint64_t *end) {
    if ((!q && q_len) || !ref_len || !has_range || !start || !end) return VCFC_E_ARG;
    return vcfc_reg::parse_query(q, q_len, ref_len, has_range, start, end);
}

int vcfc_query_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, const char *ref, uint64_t ref_len, int has_range,
                      uint64_t start, uint64_t end, uint8_t *out, uint64_t out_cap, uint64_t *out_len) {
    if (!c || (!in && n) || (!ref && ref_len) || (!out && out_cap) || !out_len) return VCFC_E_ARG;
    *out_len = 0;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    uint64_t data_off = 0, S = 0;
    int st = parse_vcfc_header(in, n, &data_off, &S);
    if (st) return st;
    BufferSink bs{out, out_cap};
    CtxDecodeBuffers B(c);
    st = vcfc_dec::query_section(in + data_off, n - data_off, S, reinterpret_cast<const uint8_t *>(ref), ref_len,
                                 has_range, start, end, B, c->stream, std::ref(bs));
    *out_len = bs.o;
    return bs.fits ? st : VCFC_E_NOSPACE;
}

int vcfc_query_file(vcfc_ctx *c, const char *in_path, const char *ref, uint64_t ref_len, int has_range,
                    uint64_t start, uint64_t end, int out_fd) {
    if (!c || !in_path || (!ref && ref_len) || out_fd < 0) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    MappedFile f;
    int st = f.open_ro(in_path);
    if (st) return st;
    uint64_t data_off = 0, S = 0;
    if ((st = parse_vcfc_header(f.p, f.n, &data_off, &S))) return st;
    CtxDecodeBuffers B(c);
    return vcfc_dec::query_section(f.p + data_off, f.n - data_off, S, reinterpret_cast<const uint8_t *>(ref), ref_len,
                                   has_range, start, end, B, c->stream, FdSink{out_fd});
}

// ---- sparse-file query: query_sparse_file_fd, reference
// src/main.cpp:235-582 ------------------------------------------------------
int vcfc_sparse_query_file(vcfc_ctx *c, const char *in_path, const char *ref, uint64_t ref_len, int has_range,
                           uint64_t start, uint64_t end, int out_fd) {
    if (!c || !in_path || (!ref && ref_len) || out_fd < 0) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    const int fd = open(in_path, O_RDONLY);
    if (fd < 0) return VCFC_E_IO;
    vcfc_dec::SparseQuery q;
    q.ref = reinterpret_cast<const uint8_t *>(ref); q.ref_len = ref_len; q.has_range = has_range;
    q.start = start; q.end = end;
    CtxDecodeBuffers B(c);
    const int st = vcfc_dec::sparse_query(fd, q, B, c->stream, FdSink{out_fd}, (c->trace & VCFC_TRACE_SPARSE_QUERY) != 0);
    close(fd);
    return st;
}

// ---- binned external index: create_binned_index4 (reference
// src/main.cpp:1284-1637), query_binned_index_binarysearch (:2974-3349);
// drivers in vcfc_index_driver.h ---------------------------------------------

uint64_t vcfc_index_workspace_size(uint64_t n_records) { return vcfc_index_workspace_layout(n_records).total; }

int vcfc_binned_index_device(const uint8_t *d_in, const uint64_t *d_rec_start, uint64_t n, uint64_t base_offset,
                             uint64_t entries_per_bin, uint8_t *d_entries, uint64_t entries_cap, uint64_t *d_count,
                             uint64_t *d_info, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream) {
    if ((n && (!d_in || !d_rec_start || !d_entries || !d_ws)) || !d_count || !d_info || !d_err || !entries_per_bin)
        return VCFC_E_ARG;
    const VcfcIndexLayout L = vcfc_index_workspace_layout(n);
    if (n && ws_bytes < L.total) return VCFC_E_NOSPACE;
    return vcfc_index_build(d_in, d_rec_start, n, base_offset, entries_per_bin, d_entries, entries_cap, d_count, d_info,
                            static_cast<uint8_t *>(d_ws), L, d_err, static_cast<hipStream_t>(stream)) == hipSuccess
               ? VCFC_OK : VCFC_E_HIP;
}

int vcfc_record_span_device(const uint8_t *d_in, const uint64_t *d_rec_start, uint64_t n, uint8_t *d_ref_idx,
                            uint64_t *d_pos, uint64_t *d_end, uint64_t *d_err, void *stream) {
    if ((n && (!d_in || !d_rec_start || !d_ref_idx || !d_pos || !d_end)) || !d_err) return VCFC_E_ARG;
    return vcfc_index_span(d_in, d_rec_start, n, d_ref_idx, d_pos, d_end, d_err, static_cast<hipStream_t>(stream)) ==
                   hipSuccess
               ? VCFC_OK : VCFC_E_HIP;
}

int vcfc_create_binned_index_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, uint64_t entries_per_bin, uint8_t *out,
                                    uint64_t out_cap, uint64_t *out_len, int64_t *err_record) {
    if (!c || (!in && n) || (!out && out_cap) || !out_len) return VCFC_E_ARG;
    *out_len = 0;
    if (err_record) *err_record = -1;
    if (!entries_per_bin) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    CtxDecodeBuffers B(c);
    std::vector<uint8_t> idx;
    const int st = vcfc_idx::create_index(in, n, entries_per_bin, B, c->stream, idx, err_record);
    if (st) return st;
    *out_len = idx.size();
    if (idx.size() > out_cap) return VCFC_E_NOSPACE;
    if (!idx.empty()) memcpy(out, idx.data(), idx.size());
    return VCFC_OK;
}

int vcfc_create_binned_index_file(vcfc_ctx *c, const char *in_path, const char *out_path, uint64_t entries_per_bin) {
    if (!c || !in_path || !out_path || !entries_per_bin) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    MappedFile f;
    int st = f.open_ro(in_path);
    if (st) return st;
    // the reference opens (truncates) the index before it reads the input and
    // writes the entries only after the last record (:1293, :1621-1628)
    const int fd = open(out_path, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fd < 0) return VCFC_E_IO;
    CtxDecodeBuffers B(c);
    std::vector<uint8_t> idx;
    st = vcfc_idx::create_index(f.p, f.n, entries_per_bin, B, c->stream, idx, nullptr);
    if (!st && !idx.empty()) st = write_all_at(fd, idx.data(), idx.size(), 0);
    if (close(fd) != 0 && !st) st = VCFC_E_IO;
    return st;
}

namespace {
struct MemReader : vcfc_idx::Reader {
    const uint8_t *p;
    uint64_t n;
    MemReader(const uint8_t *b, uint64_t size) : p(b), n(size) {}
    uint64_t size() const override { return n; }
    int64_t read(uint8_t *dst, uint64_t off, uint64_t k) override {
        if (off >= n) return 0;
        k = std::min(k, n - off);
        memcpy(dst, p + off, k);
        return (int64_t)k;
    }
};
struct FdReader : vcfc_idx::Reader {
    int fd;
    uint64_t n;
    FdReader(int f, uint64_t size) : fd(f), n(size) {}
    uint64_t size() const override { return n; }
    int64_t read(uint8_t *dst, uint64_t off, uint64_t k) override { return vcfc_dec::sq_pread(fd, dst, k, off); }
};
void trace_index(const vcfc_ctx *c, const vcfc_idx::QueryStats &qs, uint64_t fsize) {
    if (c->trace & VCFC_TRACE_INDEX)
        fprintf(stderr, "query_binned_index: %llu windows, %llu bytes read of %llu, %llu records spanned\n",
                (unsigned long long)qs.windows, (unsigned long long)qs.bytes, (unsigned long long)fsize,
                (unsigned long long)qs.records);
}
}  // namespace

int vcfc_query_binned_index_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, const uint8_t *index,
                                   uint64_t index_bytes, const char *ref, uint64_t ref_len, int has_range,
                                   uint64_t start, uint64_t end, uint8_t *out, uint64_t out_cap, uint64_t *out_len) {
    if (!c || (!in && n) || (!index && index_bytes) || (!ref && ref_len) || (!out && out_cap) || !out_len)
        return VCFC_E_ARG;
    *out_len = 0;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    BufferSink bs{out, out_cap};
    MemReader R(in, n);
    CtxDecodeBuffers B(c);
    vcfc_idx::QueryStats qs;
    const int st = vcfc_idx::query_index(R, index, index_bytes, reinterpret_cast<const uint8_t *>(ref), ref_len,
                                         has_range, start, end, B, c->stream, std::ref(bs), 4ull << 20, &qs);
    trace_index(c, qs, n);
    *out_len = bs.o;
    return bs.fits ? st : VCFC_E_NOSPACE;
}

int vcfc_query_binned_index_file(vcfc_ctx *c, const char *in_path, const char *index_path, const char *ref,
                                 uint64_t ref_len, int has_range, uint64_t start, uint64_t end, int out_fd) {
    if (!c || !in_path || !index_path || (!ref && ref_len) || out_fd < 0) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    MappedFile idx;   // the index is small: read whole
    int st = idx.open_ro(index_path);
    if (st) return st;
    const int fd = open(in_path, O_RDONLY);
    if (fd < 0) return VCFC_E_IO;
    struct stat sb;
    if (fstat(fd, &sb) != 0) { close(fd); return VCFC_E_IO; }
    FdReader R(fd, (uint64_t)sb.st_size);
    CtxDecodeBuffers B(c);
    vcfc_idx::QueryStats qs;
    st = vcfc_idx::query_index(R, idx.p, idx.n, reinterpret_cast<const uint8_t *>(ref), ref_len, has_range, start, end,
                               B, c->stream, FdSink{out_fd}, 4ull << 20, &qs);
    trace_index(c, qs, (uint64_t)sb.st_size);
    close(fd);
    return st;
}

// ---- sparse external index: create_sparse_external_index (reference
// src/main.cpp:854-999), query_sparse_external_index (:1002-1281), and
// gap_analysis (:3931-3980); drivers in vcfc_sparse_index_driver.h ------------

uint64_t vcfc_sparse_index_workspace_size(uint64_t n_records) {
    return vcfc_sparse_index_workspace_layout(n_records).total;
}

uint64_t vcfc_sparse_index_offset(uint64_t pos) { return vcfc_spx::slot_offset(pos); }

int vcfc_sparse_index_device(const uint8_t *d_in, const uint64_t *d_rec_start, uint64_t n, uint64_t base_offset,
                             uint8_t *d_entries, uint64_t *d_file_off, uint64_t *d_count, uint64_t *d_status,
                             void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream) {
    if ((n && (!d_in || !d_rec_start || !d_entries || !d_file_off || !d_ws)) || !d_count || !d_status || !d_err)
        return VCFC_E_ARG;
    const VcfcSparseIndexLayout L = vcfc_sparse_index_workspace_layout(n);
    if (n && ws_bytes < L.total) return VCFC_E_NOSPACE;
    return vcfc_sparse_index_build(d_in, d_rec_start, n, base_offset, d_entries, d_file_off, d_count, d_status,
                                   static_cast<uint8_t *>(d_ws), L, d_err, static_cast<hipStream_t>(stream)) == hipSuccess
               ? VCFC_OK : VCFC_E_HIP;
}

namespace {
struct FdIndexWriter : vcfc_spx::Writer {
    int fd;
    explicit FdIndexWriter(int f) : fd(f) {}
    int pwrite(const uint8_t *p, uint64_t k, uint64_t off) override {
        while (k) {
            const ssize_t w = ::pwrite(fd, p, k, (off_t)off);
            if (w < 0 && errno == EINTR) continue;
            if (w < 0) return errno == EINVAL || errno == EFBIG ? 1 : -1;   // past what the file system addresses
            if (w == 0) return -1;
            p += w; k -= (uint64_t)w; off += (uint64_t)w;
        }
        return 0;
    }
};
struct FdIndexFile : vcfc_spx::IndexFile {
    int fd;
    explicit FdIndexFile(int f) : fd(f) {}
    int64_t pread(uint8_t *dst, uint64_t off, uint64_t k) override { return vcfc_dec::sq_pread(fd, dst, k, off); }
    int64_t seek_data(uint64_t off) override { return (int64_t)lseek(fd, (off_t)off, SEEK_DATA); }
};
}  // namespace

int vcfc_create_sparse_index_file(vcfc_ctx *c, const char *in_path, const char *out_path, int64_t *err_record,
                                  int *seek_failed) {
    if (err_record) *err_record = -1;
    if (seek_failed) *seek_failed = 0;
    if (!c || !in_path || !out_path) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    MappedFile f;
    int st = f.open_ro(in_path);
    if (st) return st;
    // DEFAULT_FILE_CREATE_FLAGS / _MODE: opened (truncated) before the input is parsed (:863)
    const int fd = open(out_path, O_CREAT | O_TRUNC | O_RDWR, 0600);
    if (fd < 0) return VCFC_E_IO;
    CtxDecodeBuffers B(c);
    FdIndexWriter W(fd);
    vcfc_spx::CreateStats cs;
    st = vcfc_spx::create_index(f.p, f.n, B, c->stream, W, err_record, seek_failed, &cs);
    if (c->trace & VCFC_TRACE_INDEX)
        fprintf(stderr, "create_sparse_index: %llu records, %llu entries, %llu pwrite calls%s\n",
                (unsigned long long)cs.records, (unsigned long long)cs.entries, (unsigned long long)cs.pwrites,
                cs.in_order ? " (record order)" : "");
    if (close(fd) != 0 && !st) st = VCFC_E_IO;
    return st;
}

int vcfc_query_sparse_index_file(vcfc_ctx *c, const char *in_path, const char *index_path, const char *ref,
                                 uint64_t ref_len, int has_range, uint64_t start, uint64_t end, int out_fd) {
    if (!c || !in_path || !index_path || (!ref && ref_len) || out_fd < 0) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    const int fd = open(in_path, O_RDONLY);
    if (fd < 0) return VCFC_E_IO;
    const int ifd = open(index_path, O_RDONLY);
    struct stat sb;
    if (ifd < 0 || fstat(fd, &sb) != 0) {
        close(fd);
        if (ifd >= 0) close(ifd);
        return VCFC_E_IO;
    }
    FdReader R(fd, (uint64_t)sb.st_size);
    FdIndexFile I(ifd);
    CtxDecodeBuffers B(c);
    vcfc_idx::QueryStats qs;
    const int st = vcfc_spx::query_index(R, I, reinterpret_cast<const uint8_t *>(ref), ref_len, has_range, start, end, B,
                                         c->stream, FdSink{out_fd}, 4ull << 20, &qs);
    if (c->trace & VCFC_TRACE_INDEX)
        fprintf(stderr, "query_sparse_index: %llu windows, %llu bytes read of %llu, %llu records spanned\n",
                (unsigned long long)qs.windows, (unsigned long long)qs.bytes, (unsigned long long)sb.st_size,
                (unsigned long long)qs.records);
    close(ifd);
    close(fd);
    return st;
}

uint64_t vcfc_decode_sizes_workspace_size(uint64_t n_records) { return vcfc_decode_workspace_layout(n_records).total; }

int vcfc_decode_sizes_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start, uint64_t n,
                             uint64_t sample_count, uint64_t *d_line_off, uint64_t *d_pos_off, uint32_t *d_pos_len,
                             uint64_t *d_ccount, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream) {
    const bool fields = d_pos_off || d_pos_len || d_ccount;
    if ((n && (!d_in || !d_rec_start)) || !d_line_off || !d_ws || !d_err ||
        (fields && (!d_pos_off || !d_pos_len || !d_ccount)))
        return VCFC_E_ARG;
    const VcfcDecodeLayout L = vcfc_decode_workspace_layout(n);
    if (ws_bytes < L.total) return VCFC_E_NOSPACE;
    uint8_t *ws = static_cast<uint8_t *>(d_ws);
    hipStream_t s = static_cast<hipStream_t>(stream);
    VcfcDecodeArgs a;
    a.in = d_in; a.n_bytes = in_bytes; a.rec_start = d_rec_start; a.select = nullptr; a.n = n; a.S = sample_count;
    a.out = nullptr; a.out_cap = 0; a.line_off = d_line_off;
    a.st = reinterpret_cast<uint32_t *>(ws + L.st);
    a.line_size = reinterpret_cast<uint32_t *>(ws + L.line_size);
    a.end = reinterpret_cast<uint64_t *>(ws + L.end);
    a.seq_list = reinterpret_cast<uint32_t *>(ws + L.seq_list);
    a.seq_count = reinterpret_cast<uint32_t *>(ws + L.seq_count);
    a.err = d_err;   // the caller's word: the plan resets it, the field pass shares it
    a.partials = reinterpret_cast<uint64_t *>(ws + L.partials);
    if (vcfc_decode_plan(a, true, s) != hipSuccess) return VCFC_E_HIP;
    if (fields && vcfc_gap_fields(d_in, d_rec_start, n, sample_count, d_pos_off, d_pos_len, d_ccount, d_err, s) != hipSuccess)
        return VCFC_E_HIP;
    return VCFC_OK;
}

int vcfc_gap_analysis_file(vcfc_ctx *c, const char *in_path, const char *out_path) {
    if (!c || !in_path || !out_path) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    MappedFile f;
    int st = f.open_ro(in_path);
    if (st) return st;
    // the reference opens its output after the header parse (:3939-3948): a
    // header it throws on leaves no file
    uint64_t data_off = 0;
    if ((st = vcfc_dec::parse_header(f.p, f.n, &data_off, nullptr))) return st;
    const int fd = open(out_path, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fd < 0) return VCFC_E_IO;
    FileSink fs{fd};
    CtxDecodeBuffers B(c);
    st = vcfc_spx::gap_analysis(f.p, f.n, B, c->stream, std::ref(fs), nullptr);
    if (close(fd) != 0 && !st) st = VCFC_E_IO;
    return st;
}

// ---- sample subset; drivers in vcfc_subset_driver.h ---------

namespace {
// the lines (no header) of a prepared call over host bytes in[0, n): one
// region's (q), else every record's (match == nullptr) or those `match` flags
int subset_run(vcfc_ctx *c, const vcfc_sub::Call &sc, const uint8_t *in, uint64_t n, const vcfc_cnt::Query *q,
               const vcfc_dec::MatchStep *match, const vcfc_dec::Sink &sink) {
    CtxDecodeBuffers B(c);
    in += sc.data_off;
    n -= sc.data_off;
    if (q)
        return vcfc_sub::query_section(in, n, sc.S, sc.csort, sc.rank, q->ref, q->ref_len, q->has_range, q->start, q->end, B,
                                       c->stream, sink);
    if (match) return vcfc_sub::matched_section(in, n, sc.S, sc.csort, sc.rank, *match, B, c->stream, sink);
    return vcfc_sub::decode_section(in, n, sc.S, sc.csort, sc.rank, B, c->stream, sink);
}

// header: the subset's header goes first (the whole-file decode)
int subset_to_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, const uint32_t *cols, uint64_t n_cols, bool header,
                     const vcfc_cnt::Query *q, const vcfc_dec::MatchStep *match, uint8_t *out, uint64_t out_cap,
                     uint64_t *out_len) {
    *out_len = 0;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    vcfc_sub::Call sc;
    int st = sc.prepare(in, n, cols, n_cols);
    if (st) return st;
    BufferSink bs{out, out_cap};
    if (header) bs(sc.hdr.data(), sc.hdr.size());
    st = subset_run(c, sc, in, n, q, match, std::ref(bs));
    *out_len = bs.o;
    return bs.fits ? st : VCFC_E_NOSPACE;
}

int subset_to_fd(vcfc_ctx *c, const char *in_path, const uint32_t *cols, uint64_t n_cols, const vcfc_cnt::Query *q,
                 const vcfc_dec::MatchStep *match, int out_fd) {
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    MappedFile f;
    int st = f.open_ro(in_path);
    if (st) return st;
    vcfc_sub::Call sc;
    if ((st = sc.prepare(f.p, f.n, cols, n_cols))) return st;
    return subset_run(c, sc, f.p, f.n, q, match, FdSink{out_fd});
}
}  // namespace

int vcfc_sample_columns(const uint8_t *in, uint64_t n, const char *names, uint64_t names_len, uint32_t *cols,
                        uint64_t cols_cap, uint64_t *n_cols, uint64_t *bad_off) {
    if ((!in && n) || (!names && names_len) || (!cols && cols_cap) || !n_cols || !bad_off) return VCFC_E_ARG;
    *n_cols = 0;
    *bad_off = 0;
    return vcfc_sub::sample_columns(in, n, names, names_len, cols, cols_cap, n_cols, bad_off);
}

int vcfc_decompress_samples_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, const uint32_t *cols, uint64_t n_cols,
                                   uint8_t *out, uint64_t out_cap, uint64_t *out_len) {
    if (!c || (!in && n) || (!out && out_cap) || !out_len) return VCFC_E_ARG;
    return subset_to_buffer(c, in, n, cols, n_cols, true, nullptr, nullptr, out, out_cap, out_len);
}

int vcfc_decompress_samples_file(vcfc_ctx *c, const char *in_path, const char *out_path, const uint32_t *cols,
                                 uint64_t n_cols) {
    if (!c || !in_path || !out_path) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    MappedFile f;
    int st = f.open_ro(in_path);
    if (st) return st;
    vcfc_sub::Call sc;
    if ((st = sc.prepare(f.p, f.n, cols, n_cols))) return st;   // nothing written: the output is opened after this
    const int fd = open(out_path, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fd < 0) return VCFC_E_IO;
    FileSink fs{fd};
    st = fs(sc.hdr.data(), sc.hdr.size()) ? subset_run(c, sc, f.p, f.n, nullptr, nullptr, std::ref(fs)) : VCFC_E_IO;
    if (close(fd) != 0 && !st) st = VCFC_E_IO;
    return st;
}

int vcfc_query_samples_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, const char *ref, uint64_t ref_len,
                              int has_range, uint64_t start, uint64_t end, const uint32_t *cols, uint64_t n_cols,
                              uint8_t *out, uint64_t out_cap, uint64_t *out_len) {
    if (!c || (!in && n) || (!ref && ref_len) || (!out && out_cap) || !out_len) return VCFC_E_ARG;
    const vcfc_cnt::Query q{reinterpret_cast<const uint8_t *>(ref), ref_len, has_range, start, end};
    return subset_to_buffer(c, in, n, cols, n_cols, false, &q, nullptr, out, out_cap, out_len);
}

int vcfc_query_samples_file(vcfc_ctx *c, const char *in_path, const char *ref, uint64_t ref_len, int has_range,
                            uint64_t start, uint64_t end, const uint32_t *cols, uint64_t n_cols, int out_fd) {
    if (!c || !in_path || (!ref && ref_len) || out_fd < 0) return VCFC_E_ARG;
    const vcfc_cnt::Query q{reinterpret_cast<const uint8_t *>(ref), ref_len, has_range, start, end};
    return subset_to_fd(c, in_path, cols, n_cols, &q, nullptr, out_fd);
}

uint64_t vcfc_subset_workspace_size(uint64_t n_records, uint64_t n_cols) {
    return vcfc_subset_workspace_layout(n_records, n_cols).total;
}

int vcfc_decode_samples_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start,
                               const uint8_t *d_select, uint64_t n, uint64_t samples, const uint32_t *cols,
                               uint64_t n_cols, uint8_t *d_out, uint64_t out_cap, uint64_t *d_line_off, void *d_ws,
                               uint64_t ws_bytes, uint64_t *d_err, void *stream) {
    if ((n && (!d_in || !d_rec_start || !d_out)) || !d_ws || !d_line_off || !d_err) return VCFC_E_ARG;
    std::vector<uint32_t> csort, rank;
    if (vcfc_sub::sort_columns(cols, n_cols, samples, csort, rank)) return VCFC_E_ARG;
    return vcfc_sub::records_device(vcfc_sub::SUBSET, d_in, in_bytes, d_rec_start, d_select, n, samples, csort, rank, d_out,
                                    out_cap, d_line_off, d_ws, ws_bytes, d_err, static_cast<hipStream_t>(stream));
}

// ---- genotype counts; driver in vcfc_counts_driver.h -----------

uint64_t vcfc_counts_workspace_size(uint64_t n_records, uint64_t samples) {
    return vcfc_counts_workspace_layout(n_records, samples).total;
}

uint64_t vcfc_counts_lds_samples(void) { return VCFC_COUNTS_LDS_SAMPLES; }

uint64_t vcfc_counts_trip_records(uint64_t samples, int with_sample_table) {
    return vcfc_counts_scan_trip(samples, with_sample_table != 0);
}

int vcfc_genotype_counts_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start,
                                const uint8_t *d_select, uint64_t n, uint64_t samples, uint32_t *d_variant,
                                uint64_t *d_sample, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream) {
    return vcfc_cnt::counts_device(d_in, in_bytes, d_rec_start, d_select, n, samples, d_variant, d_sample, d_ws, ws_bytes,
                                   d_err, static_cast<hipStream_t>(stream));
}

namespace {
// what the two genotype-counts buffer entries hand back from a Result
int counts_to_caller(int st, const vcfc_cnt::Result &R, uint64_t S, uint64_t *rec_index, uint32_t *rows, uint64_t rows_cap,
                     uint64_t *n_rows, uint64_t *sample_table, uint64_t sample_cap, uint64_t *n_samples,
                     uint64_t *err_record) {
    if (st != VCFC_OK && st != VCFC_E_FORMAT) return st;
    *n_rows = R.index.size();
    *n_samples = st == VCFC_OK ? S : 0;
    *err_record = R.err_record;
    if (*n_rows > rows_cap || *n_samples > sample_cap) return VCFC_E_NOSPACE;
    if (*n_rows) {
        memcpy(rec_index, R.index.data(), 8 * R.index.size());
        memcpy(rows, R.rows.data(), 4 * R.rows.size());
    }
    if (st == VCFC_OK) memcpy(sample_table, R.samples.data(), 8 * R.samples.size());
    return st;
}

// the two files of a genotype-counts file entry; run(f, R, &data_off, &S) counts
int counts_to_files(const char *in_path, const char *variants_path, const char *samples_path,
                    const std::function<int(const MappedFile &, vcfc_cnt::Result &, uint64_t *, uint64_t *)> &run) {
    const int vfd = open(variants_path, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (vfd < 0) return VCFC_E_IO;
    const int sfd = open(samples_path, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (sfd < 0) {
        close(vfd);
        return VCFC_E_IO;
    }
    MappedFile f;
    int st = f.open_ro(in_path);
    if (!st) {
        vcfc_cnt::Result R;
        uint64_t data_off = 0, S = 0;
        st = run(f, R, &data_off, &S);
        if (data_off && S && (st == VCFC_OK || st == VCFC_E_FORMAT)) {   // past the header
            std::vector<uint8_t> text;
            vcfc_cnt::render_variants(f.p + data_off, R, text);
            if (write_all_at(vfd, text.data(), text.size(), 0)) st = VCFC_E_IO;
            if (st == VCFC_OK) {
                vcfc_cnt::render_samples(f.p, data_off, S, R, text);
                if (write_all_at(sfd, text.data(), text.size(), 0)) st = VCFC_E_IO;
            }
        }
    }
    if (close(vfd) != 0 && !st) st = VCFC_E_IO;
    if (close(sfd) != 0 && !st) st = VCFC_E_IO;
    return st;
}
}  // namespace

int vcfc_genotype_counts_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, int has_query, const char *ref,
                                uint64_t ref_len, int has_range, uint64_t start, uint64_t end, uint64_t *rec_index,
                                uint32_t *rows, uint64_t rows_cap, uint64_t *n_rows, uint64_t *sample_table,
                                uint64_t sample_cap, uint64_t *n_samples, uint64_t *err_record) {
    if (!c || (!in && n) || (has_query && !ref && ref_len) || ((!rec_index || !rows) && rows_cap) ||
        (!sample_table && sample_cap) || !n_rows || !n_samples || !err_record)
        return VCFC_E_ARG;
    *n_rows = *n_samples = 0;
    *err_record = ~0ull;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    const vcfc_cnt::Query q{reinterpret_cast<const uint8_t *>(ref), ref_len, has_range, start, end};
    vcfc_cnt::Result R;
    uint64_t data_off = 0, S = 0;
    CtxDecodeBuffers B(c);
    const int st = vcfc_cnt::counts_file(in, n, has_query ? &q : nullptr, B, c->stream, R, &data_off, &S);
    return counts_to_caller(st, R, S, rec_index, rows, rows_cap, n_rows, sample_table, sample_cap, n_samples, err_record);
}

int vcfc_genotype_counts_file(vcfc_ctx *c, const char *in_path, const char *variants_path, const char *samples_path,
                              int has_query, const char *ref, uint64_t ref_len, int has_range, uint64_t start,
                              uint64_t end) {
    if (!c || !in_path || !variants_path || !samples_path || (has_query && !ref && ref_len)) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    const vcfc_cnt::Query q{reinterpret_cast<const uint8_t *>(ref), ref_len, has_range, start, end};
    return counts_to_files(in_path, variants_path, samples_path,
                           [&](const MappedFile &f, vcfc_cnt::Result &R, uint64_t *data_off, uint64_t *S) {
                               CtxDecodeBuffers B(c);
                               return vcfc_cnt::counts_file(f.p, f.n, has_query ? &q : nullptr, B, c->stream, R, data_off, S);
                           });
}

// ---- region-list queries; drivers in vcfc_regions_driver.h ----

int vcfc_regions_build(const char *text, uint64_t len, uint8_t *table, uint64_t table_cap, uint64_t *table_bytes,
                       uint64_t *n_regions, uint64_t *bad_line) {
    if ((!text && len) || (!table && table_cap) || !table_bytes || !n_regions || !bad_line) return VCFC_E_ARG;
    return vcfc_reg::regions_build(text, len, table, table_cap, table_bytes, n_regions, bad_line);
}

uint64_t vcfc_regions_workspace_size(uint64_t table_bytes) { return vcfc_reg::regions_workspace_size(table_bytes); }

int vcfc_regions_upload(const uint8_t *table, uint64_t table_bytes, void *d_ws, uint64_t ws_bytes, void *stream) {
    return vcfc_reg::regions_upload(table, table_bytes, d_ws, ws_bytes, static_cast<hipStream_t>(stream));
}

int vcfc_regions_match_device(const uint8_t *d_in, const uint64_t *d_rec_start, uint64_t n, const void *d_ws,
                              uint64_t ws_bytes, uint8_t *d_flag, uint64_t *d_err, void *stream) {
    return vcfc_reg::regions_match_device(d_in, d_rec_start, n, d_ws, ws_bytes, d_flag, d_err,
                                          static_cast<hipStream_t>(stream));
}

int vcfc_query_regions_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, const uint8_t *table, uint64_t table_bytes,
                              uint8_t *out, uint64_t out_cap, uint64_t *out_len) {
    if (!c || (!in && n) || (!out && out_cap) || !out_len || !vcfc_reg::regions_validate(table, table_bytes))
        return VCFC_E_ARG;
    *out_len = 0;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    uint64_t data_off = 0, S = 0;
    int st = parse_vcfc_header(in, n, &data_off, &S);
    if (st) return st;
    BufferSink bs{out, out_cap};
    const uint8_t *d_table = nullptr;
    CtxDecodeBuffers B(c);
    st = vcfc_dec::query_regions_section(in + data_off, n - data_off, S, vcfc_reg::regions_step(table, table_bytes, &d_table),
                                         B, c->stream, std::ref(bs));
    *out_len = bs.o;
    return bs.fits ? st : VCFC_E_NOSPACE;
}

int vcfc_query_regions_file(vcfc_ctx *c, const char *in_path, const uint8_t *table, uint64_t table_bytes, int out_fd) {
    if (!c || !in_path || out_fd < 0 || !vcfc_reg::regions_validate(table, table_bytes)) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    MappedFile f;
    int st = f.open_ro(in_path);
    if (st) return st;
    uint64_t data_off = 0, S = 0;
    if ((st = parse_vcfc_header(f.p, f.n, &data_off, &S))) return st;
    const uint8_t *d_table = nullptr;
    CtxDecodeBuffers B(c);
    return vcfc_dec::query_regions_section(f.p + data_off, f.n - data_off, S,
                                           vcfc_reg::regions_step(table, table_bytes, &d_table), B, c->stream, FdSink{out_fd});
}

int vcfc_query_samples_regions_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, const uint8_t *table,
                                      uint64_t table_bytes, const uint32_t *cols, uint64_t n_cols, uint8_t *out,
                                      uint64_t out_cap, uint64_t *out_len) {
    if (!c || (!in && n) || (!out && out_cap) || !out_len || !vcfc_reg::regions_validate(table, table_bytes))
        return VCFC_E_ARG;
    const uint8_t *d_table = nullptr;
    const vcfc_dec::MatchStep m = vcfc_reg::regions_step(table, table_bytes, &d_table);
    return subset_to_buffer(c, in, n, cols, n_cols, false, nullptr, &m, out, out_cap, out_len);
}

int vcfc_query_samples_regions_file(vcfc_ctx *c, const char *in_path, const uint8_t *table, uint64_t table_bytes,
                                    const uint32_t *cols, uint64_t n_cols, int out_fd) {
    if (!c || !in_path || out_fd < 0 || !vcfc_reg::regions_validate(table, table_bytes)) return VCFC_E_ARG;
    const uint8_t *d_table = nullptr;
    const vcfc_dec::MatchStep m = vcfc_reg::regions_step(table, table_bytes, &d_table);
    return subset_to_fd(c, in_path, cols, n_cols, nullptr, &m, out_fd);
}

// ---- extract; driver in vcfc_extract_driver.h ---------------------

uint64_t vcfc_extract_bound(uint64_t in_bytes, uint64_t n_records, uint64_t n_cols) {
    return vcfc_ext::extract_bound(in_bytes, n_records, n_cols);
}

namespace {
// header (sunk first) and records of an extract of host bytes in[0, n)
int extract_run(vcfc_ctx *c, const uint8_t *in, uint64_t n, const uint32_t *cols, uint64_t n_cols,
                const vcfc_dec::MatchStep *match, const vcfc_dec::Sink &sink) {
    vcfc_ext::Call ec;
    const int st = ec.prepare(in, n, cols, n_cols);
    if (st) return st;   // nothing written
    if (!sink(ec.hdr.data(), ec.hdr.size())) return VCFC_E_IO;
    CtxDecodeBuffers B(c);
    return vcfc_ext::extract_section(in + ec.data_off, n - ec.data_off, ec.S, ec.csort, ec.rank, match, B, c->stream, sink);
}

int extract_to_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, const uint32_t *cols, uint64_t n_cols,
                      const vcfc_dec::MatchStep *match, uint8_t *out, uint64_t out_cap, uint64_t *out_len) {
    *out_len = 0;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    BufferSink bs{out, out_cap};
    const int st = extract_run(c, in, n, cols, n_cols, match, std::ref(bs));
    *out_len = bs.o;
    return bs.fits ? st : VCFC_E_NOSPACE;
}

// (the output is created before the input is parsed)
int extract_to_file(vcfc_ctx *c, const char *in_path, const char *out_path, const uint32_t *cols, uint64_t n_cols,
                    const vcfc_dec::MatchStep *match) {
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    MappedFile f;
    int st = f.open_ro(in_path);
    if (st) return st;
    const int fd = open(out_path, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fd < 0) return VCFC_E_IO;
    st = extract_run(c, f.p, f.n, cols, n_cols, match, FdSink{fd});
    if (close(fd) != 0 && !st) st = VCFC_E_IO;
    return st;
}
}  // namespace

int vcfc_extract_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, const uint32_t *cols, uint64_t n_cols, int has_query,
                        const char *ref, uint64_t ref_len, int has_range, uint64_t start, uint64_t end, uint8_t *out,
                        uint64_t out_cap, uint64_t *out_len) {
    if (!c || (!in && n) || (has_query && !ref && ref_len) || (!out && out_cap) || !out_len) return VCFC_E_ARG;
    if (has_query && ref_len > 0xFFFFFFFFull) return VCFC_E_FORMAT;
    VcfcQuery q;
    const vcfc_dec::MatchStep m =
        vcfc_dec::region_step(reinterpret_cast<const uint8_t *>(ref), has_query ? ref_len : 0, has_range, start, end, &q);
    return extract_to_buffer(c, in, n, cols, n_cols, has_query ? &m : nullptr, out, out_cap, out_len);
}

int vcfc_extract_file(vcfc_ctx *c, const char *in_path, const char *out_path, const uint32_t *cols, uint64_t n_cols,
                      int has_query, const char *ref, uint64_t ref_len, int has_range, uint64_t start, uint64_t end) {
    if (!c || !in_path || !out_path || (has_query && !ref && ref_len)) return VCFC_E_ARG;
    if (has_query && ref_len > 0xFFFFFFFFull) return VCFC_E_FORMAT;
    VcfcQuery q;
    const vcfc_dec::MatchStep m =
        vcfc_dec::region_step(reinterpret_cast<const uint8_t *>(ref), has_query ? ref_len : 0, has_range, start, end, &q);
    return extract_to_file(c, in_path, out_path, cols, n_cols, has_query ? &m : nullptr);
}

int vcfc_extract_regions_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, const uint32_t *cols, uint64_t n_cols,
                                const uint8_t *table, uint64_t table_bytes, uint8_t *out, uint64_t out_cap,
                                uint64_t *out_len) {
    if (!c || (!in && n) || (!out && out_cap) || !out_len || !vcfc_reg::regions_validate(table, table_bytes))
        return VCFC_E_ARG;
    const uint8_t *d_table = nullptr;
    const vcfc_dec::MatchStep m = vcfc_reg::regions_step(table, table_bytes, &d_table);
    return extract_to_buffer(c, in, n, cols, n_cols, &m, out, out_cap, out_len);
}

int vcfc_extract_regions_file(vcfc_ctx *c, const char *in_path, const char *out_path, const uint32_t *cols,
                              uint64_t n_cols, const uint8_t *table, uint64_t table_bytes) {
    if (!c || !in_path || !out_path || !vcfc_reg::regions_validate(table, table_bytes)) return VCFC_E_ARG;
    const uint8_t *d_table = nullptr;
    const vcfc_dec::MatchStep m = vcfc_reg::regions_step(table, table_bytes, &d_table);
    return extract_to_file(c, in_path, out_path, cols, n_cols, &m);
}

static_assert(VCFC_EXTRACT_TILE_COLS == VCFC_EXTRACT_TILE, "include/vcfc.h states the kernels' tile limit");

uint64_t vcfc_extract_workspace_size(uint64_t n_records, uint64_t n_cols) {
    return vcfc_extract_workspace_layout(n_records, n_cols).total;
}

int vcfc_extract_samples_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start,
                                const uint8_t *d_select, uint64_t n, uint64_t samples, const uint32_t *cols,
                                uint64_t n_cols, uint8_t *d_out, uint64_t out_cap, uint64_t *d_rec_off, void *d_ws,
                                uint64_t ws_bytes, uint64_t *d_err, void *stream) {
    if ((n && (!d_in || !d_rec_start || (!d_out && out_cap))) || !d_ws || !d_rec_off || !d_err) return VCFC_E_ARG;
    std::vector<uint32_t> csort, rank;
    if (vcfc_ext::device_columns(cols, n_cols, samples, csort, rank)) return VCFC_E_ARG;
    return vcfc_sub::records_device(vcfc_ext::EXTRACT, d_in, in_bytes, d_rec_start, d_select, n, samples, csort, rank, d_out,
                                    out_cap, d_rec_off, d_ws, ws_bytes, d_err, static_cast<hipStream_t>(stream));
}

int vcfc_genotype_counts_regions_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, const uint8_t *table,
                                        uint64_t table_bytes, uint64_t *rec_index, uint32_t *rows, uint64_t rows_cap,
                                        uint64_t *n_rows, uint64_t *sample_table, uint64_t sample_cap, uint64_t *n_samples,
                                        uint64_t *err_record) {
    if (!c || (!in && n) || ((!rec_index || !rows) && rows_cap) || (!sample_table && sample_cap) || !n_rows ||
        !n_samples || !err_record || !vcfc_reg::regions_validate(table, table_bytes))
        return VCFC_E_ARG;
    *n_rows = *n_samples = 0;
    *err_record = ~0ull;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    const uint8_t *d_table = nullptr;
    const vcfc_dec::MatchStep match = vcfc_reg::regions_step(table, table_bytes, &d_table);
    vcfc_cnt::Result R;
    uint64_t data_off = 0, S = 0;
    CtxDecodeBuffers B(c);
    const int st = vcfc_cnt::counts_file(in, n, &match, B, c->stream, R, &data_off, &S);
    return counts_to_caller(st, R, S, rec_index, rows, rows_cap, n_rows, sample_table, sample_cap, n_samples, err_record);
}

int vcfc_genotype_counts_regions_file(vcfc_ctx *c, const char *in_path, const char *variants_path,
                                      const char *samples_path, const uint8_t *table, uint64_t table_bytes) {
    if (!c || !in_path || !variants_path || !samples_path || !vcfc_reg::regions_validate(table, table_bytes))
        return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    const uint8_t *d_table = nullptr;
    const vcfc_dec::MatchStep match = vcfc_reg::regions_step(table, table_bytes, &d_table);
    return counts_to_files(in_path, variants_path, samples_path,
                           [&](const MappedFile &f, vcfc_cnt::Result &R, uint64_t *data_off, uint64_t *S) {
                               CtxDecodeBuffers B(c);
                               return vcfc_cnt::counts_file(f.p, f.n, &match, B, c->stream, R, data_off, S);
                           });
}

// ---- genotype matrix; driver in vcfc_matrix_driver.h -----------

uint64_t vcfc_matrix_row_bytes(int layout, uint64_t samples) { return vcfc_matrix_row_size(layout, samples); }

uint64_t vcfc_matrix_lds_samples(int layout) { return vcfc_matrix_tile_samples(layout); }

uint64_t vcfc_matrix_trip_records(int layout) { return vcfc_matrix_scan_trip(layout); }

uint64_t vcfc_matrix_workspace_size(uint64_t n_records, uint64_t, int) {
    return vcfc_matrix_workspace_layout(n_records).total;
}

int vcfc_genotype_matrix_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start,
                                const uint8_t *d_select, uint64_t n, uint64_t samples, int layout, uint8_t *d_out,
                                uint64_t out_cap, uint64_t row_stride, uint64_t *d_row_of, void *d_ws, uint64_t ws_bytes,
                                uint64_t *d_err, void *stream) {
    return vcfc_gm::matrix_device(d_in, in_bytes, d_rec_start, d_select, n, samples, layout, d_out, out_cap, row_stride,
                                  d_row_of, d_ws, ws_bytes, d_err, static_cast<hipStream_t>(stream));
}

namespace {
// run(in, n, B, R, &data_off, &S): the matrix of a .vcfc by one of the two match steps
using MatrixRun = std::function<int(const uint8_t *, uint64_t, vcfc_dec::Buffers &, vcfc_gm::Result &, uint64_t *, uint64_t *)>;

// what the two genotype-matrix buffer entries hand back
int matrix_to_caller(vcfc_ctx *c, const uint8_t *in, uint64_t n, int layout, uint64_t *rec_index, uint64_t rows_cap, uint8_t *rows, uint64_t rows_bytes,
                     uint64_t *n_rows, uint64_t *n_samples, uint64_t *err_record, const MatrixRun &run) {
    if (!c || (!in && n) || (!rec_index && rows_cap) || (!rows && rows_bytes) || !n_rows || !n_samples || !err_record) return VCFC_E_ARG;
    *n_rows = *n_samples = 0;
    *err_record = ~0ull;
    if (!vcfc_matrix_row_size(layout, 1)) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    vcfc_gm::Result R;
    uint64_t data_off = 0, S = 0;
    CtxDecodeBuffers B(c);
    const int st = run(in, n, B, R, &data_off, &S);
    if (st != VCFC_OK && st != VCFC_E_FORMAT) return st;
    *n_rows = R.index.size();
    *n_samples = S;
    *err_record = R.err_record;
    if (*n_rows > rows_cap || R.rows.size() > rows_bytes) return VCFC_E_NOSPACE;
    if (*n_rows) {
        memcpy(rec_index, R.index.data(), 8 * R.index.size());
        memcpy(rows, R.rows.data(), R.rows.size());
    }
    return st;
}

// the three files of an export-bed entry
int matrix_to_files(vcfc_ctx *c, const char *in_path, const char *prefix, const MatrixRun &run) {
    const std::string p(prefix);
    int fd[3] = {-1, -1, -1};
    static const char *const ext[3] = {".bed", ".bim", ".fam"};
    for (int k = 0; k < 3; k++) {
        fd[k] = open((p + ext[k]).c_str(), O_CREAT | O_TRUNC | O_WRONLY, 0644);
        if (fd[k] < 0) {
            while (k-- > 0) close(fd[k]);
            return VCFC_E_IO;
        }
    }
    MappedFile f;
    int st = f.open_ro(in_path);
    if (!st) {
        vcfc_gm::Result R;
        uint64_t data_off = 0, S = 0;
        CtxDecodeBuffers B(c);
        st = run(f.p, f.n, B, R, &data_off, &S);
        if (data_off && S && (st == VCFC_OK || st == VCFC_E_FORMAT)) {   // past the header
            std::vector<uint8_t> text;
            vcfc_gm::render_bed(R, text);
            if (write_all_at(fd[0], text.data(), text.size(), 0)) st = VCFC_E_IO;
            vcfc_gm::render_bim(f.p + data_off, R, text);
            if (write_all_at(fd[1], text.data(), text.size(), 0)) st = VCFC_E_IO;
            if (st == VCFC_OK) {
                vcfc_gm::render_fam(f.p, data_off, S, text);
                if (write_all_at(fd[2], text.data(), text.size(), 0)) st = VCFC_E_IO;
            }
        }
    }
    for (int k = 0; k < 3; k++)
        if (close(fd[k]) != 0 && !st) st = VCFC_E_IO;
    return st;
}
}  // namespace

int vcfc_genotype_matrix_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, int layout, int has_query, const char *ref,
                                uint64_t ref_len, int has_range, uint64_t start, uint64_t end, uint64_t *rec_index,
                                uint64_t rows_cap, uint8_t *rows, uint64_t rows_bytes, uint64_t *n_rows,
                                uint64_t *n_samples, uint64_t *err_record) {
    if (has_query && !ref && ref_len) return VCFC_E_ARG;
    const vcfc_gm::Query q{reinterpret_cast<const uint8_t *>(ref), ref_len, has_range, start, end};
    return matrix_to_caller(c, in, n, layout, rec_index, rows_cap, rows, rows_bytes, n_rows, n_samples, err_record,
                            [&](const uint8_t *p, uint64_t pn, vcfc_dec::Buffers &B, vcfc_gm::Result &R, uint64_t *data_off,
                                uint64_t *S) {
                                return vcfc_gm::matrix_file(p, pn, layout, has_query ? &q : nullptr, B, c->stream, R, data_off, S);
                            });
}

int vcfc_genotype_matrix_regions_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, int layout, const uint8_t *table,
                                        uint64_t table_bytes, uint64_t *rec_index, uint64_t rows_cap, uint8_t *rows,
                                        uint64_t rows_bytes, uint64_t *n_rows, uint64_t *n_samples, uint64_t *err_record) {
    if (!vcfc_reg::regions_validate(table, table_bytes)) return VCFC_E_ARG;
    const uint8_t *d_table = nullptr;
    const vcfc_dec::MatchStep match = vcfc_reg::regions_step(table, table_bytes, &d_table);
    return matrix_to_caller(c, in, n, layout, rec_index, rows_cap, rows, rows_bytes, n_rows, n_samples, err_record,
                            [&](const uint8_t *p, uint64_t pn, vcfc_dec::Buffers &B, vcfc_gm::Result &R, uint64_t *data_off,
                                uint64_t *S) { return vcfc_gm::matrix_file(p, pn, layout, &match, B, c->stream, R, data_off, S); });
}

int vcfc_export_bed_file(vcfc_ctx *c, const char *in_path, const char *prefix, int has_query, const char *ref,
                         uint64_t ref_len, int has_range, uint64_t start, uint64_t end) {
    if (!c || !in_path || !prefix || (has_query && !ref && ref_len)) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    const vcfc_gm::Query q{reinterpret_cast<const uint8_t *>(ref), ref_len, has_range, start, end};
    return matrix_to_files(c, in_path, prefix,
                           [&](const uint8_t *p, uint64_t pn, vcfc_dec::Buffers &B, vcfc_gm::Result &R, uint64_t *data_off,
                               uint64_t *S) {
                               return vcfc_gm::matrix_file(p, pn, VCFC_MATRIX_BED, has_query ? &q : nullptr, B, c->stream, R,
                                                           data_off, S);
                           });
}

int vcfc_export_bed_regions_file(vcfc_ctx *c, const char *in_path, const char *prefix, const uint8_t *table,
                                 uint64_t table_bytes) {
    if (!c || !in_path || !prefix || !vcfc_reg::regions_validate(table, table_bytes)) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    const uint8_t *d_table = nullptr;
    const vcfc_dec::MatchStep match = vcfc_reg::regions_step(table, table_bytes, &d_table);
    return matrix_to_files(c, in_path, prefix,
                           [&](const uint8_t *p, uint64_t pn, vcfc_dec::Buffers &B, vcfc_gm::Result &R, uint64_t *data_off,
                               uint64_t *S) {
                               return vcfc_gm::matrix_file(p, pn, VCFC_MATRIX_BED, &match, B, c->stream, R, data_off, S);
                           });
}

// ---- LD window; driver in vcfc_ld_driver.h -----------------------

uint64_t vcfc_ld_workspace_size(uint64_t n_records, uint64_t samples, uint64_t) {
    return vcfc_ld_workspace_layout(n_records, samples).total;
}

int vcfc_ld_tables_device(const uint8_t *d_bed, uint64_t n_rows, uint64_t row_stride, uint64_t samples, uint64_t window,
                          uint32_t *d_tables, uint64_t pairs_cap, void *d_ws, uint64_t ws_bytes, uint64_t *d_err,
                          void *stream) {
    return vcfc_ld::tables_device(d_bed, n_rows, row_stride, samples, window, d_tables, pairs_cap, d_ws, ws_bytes, d_err,
                                  static_cast<hipStream_t>(stream));
}

int vcfc_ld_window_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start, const uint8_t *d_select,
                          uint64_t n, uint64_t samples, uint64_t window, uint32_t *d_tables, uint64_t pairs_cap,
                          uint64_t *d_row_of, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream) {
    return vcfc_ld::window_device(d_in, in_bytes, d_rec_start, d_select, n, samples, window, d_tables, pairs_cap, d_row_of,
                                  d_ws, ws_bytes, d_err, static_cast<hipStream_t>(stream));
}

namespace {
// run(in, n, B, R, &data_off, &S): the band of a .vcfc by one of the two match steps
using LdRun = std::function<int(const uint8_t *, uint64_t, vcfc_dec::Buffers &, vcfc_ld::Result &, uint64_t *, uint64_t *)>;

// what the two ld-window buffer entries hand back
int ld_to_caller(vcfc_ctx *c, const uint8_t *in, uint64_t n, uint64_t window, uint64_t *rec_index, uint64_t rows_cap,
                 uint32_t *tables, uint64_t pairs_cap, uint64_t *n_rows, uint64_t *err_record, const LdRun &run) {
    if (!c || (!in && n) || (!rec_index && rows_cap) || (!tables && pairs_cap) || !n_rows || !err_record) return VCFC_E_ARG;
    *n_rows = 0;
    *err_record = ~0ull;
    if (window == 0 || window >= (1ull << 16)) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    vcfc_ld::Result R;
    uint64_t data_off = 0, S = 0;
    CtxDecodeBuffers B(c);
    const int st = run(in, n, B, R, &data_off, &S);
    if (st != VCFC_OK && st != VCFC_E_FORMAT) return st;
    *n_rows = R.index.size();
    *err_record = R.err_record;
    if (*n_rows > rows_cap || R.tables.size() / 9 > pairs_cap) return VCFC_E_NOSPACE;
    if (*n_rows) {
        memcpy(rec_index, R.index.data(), 8 * R.index.size());
        memcpy(tables, R.tables.data(), 4 * R.tables.size());
    }
    return st;
}

// the text file of an ld-window entry
int ld_to_file(vcfc_ctx *c, const char *in_path, const char *out_path, uint64_t window, double min_r2, const LdRun &run) {
    const int fd = open(out_path, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fd < 0) return VCFC_E_IO;
    MappedFile f;
    int st = f.open_ro(in_path);
    if (!st) {
        vcfc_ld::Result R;
        uint64_t data_off = 0, S = 0;
        CtxDecodeBuffers B(c);
        st = run(f.p, f.n, B, R, &data_off, &S);
        if (data_off && S && (st == VCFC_OK || st == VCFC_E_FORMAT)) {   // past the header
            std::vector<uint8_t> text;
            vcfc_ld::render_tsv(f.p + data_off, R, window, min_r2, text);
            if (write_all_at(fd, text.data(), text.size(), 0)) st = VCFC_E_IO;
        }
    }
    if (close(fd) != 0 && !st) st = VCFC_E_IO;
    return st;
}
}  // namespace

int vcfc_ld_window_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, uint64_t window, int has_query, const char *ref,
                          uint64_t ref_len, int has_range, uint64_t start, uint64_t end, uint64_t *rec_index,
                          uint64_t rows_cap, uint32_t *tables, uint64_t pairs_cap, uint64_t *n_rows, uint64_t *err_record) {
    if (has_query && !ref && ref_len) return VCFC_E_ARG;
    const vcfc_ld::Query q{reinterpret_cast<const uint8_t *>(ref), ref_len, has_range, start, end};
    return ld_to_caller(c, in, n, window, rec_index, rows_cap, tables, pairs_cap, n_rows, err_record,
                        [&](const uint8_t *p, uint64_t pn, vcfc_dec::Buffers &B, vcfc_ld::Result &R, uint64_t *data_off,
                            uint64_t *S) {
                            return vcfc_ld::window_file(p, pn, window, has_query ? &q : nullptr, B, c->stream, R, data_off, S);
                        });
}

int vcfc_ld_window_regions_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, uint64_t window, const uint8_t *table,
                                  uint64_t table_bytes, uint64_t *rec_index, uint64_t rows_cap, uint32_t *tables,
                                  uint64_t pairs_cap, uint64_t *n_rows, uint64_t *err_record) {
    if (!vcfc_reg::regions_validate(table, table_bytes)) return VCFC_E_ARG;
    const uint8_t *d_table = nullptr;
    const vcfc_dec::MatchStep match = vcfc_reg::regions_step(table, table_bytes, &d_table);
    return ld_to_caller(c, in, n, window, rec_index, rows_cap, tables, pairs_cap, n_rows, err_record,
                        [&](const uint8_t *p, uint64_t pn, vcfc_dec::Buffers &B, vcfc_ld::Result &R, uint64_t *data_off,
                            uint64_t *S) { return vcfc_ld::window_file(p, pn, window, &match, B, c->stream, R, data_off, S); });
}

int vcfc_ld_window_file(vcfc_ctx *c, const char *in_path, const char *out_tsv, uint64_t window, double min_r2,
                        int has_query, const char *ref, uint64_t ref_len, int has_range, uint64_t start, uint64_t end) {
    if (!c || !in_path || !out_tsv || (has_query && !ref && ref_len) || window == 0 || window >= (1ull << 16))
        return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    const vcfc_ld::Query q{reinterpret_cast<const uint8_t *>(ref), ref_len, has_range, start, end};
    return ld_to_file(c, in_path, out_tsv, window, min_r2,
                      [&](const uint8_t *p, uint64_t pn, vcfc_dec::Buffers &B, vcfc_ld::Result &R, uint64_t *data_off,
                          uint64_t *S) {
                          return vcfc_ld::window_file(p, pn, window, has_query ? &q : nullptr, B, c->stream, R, data_off, S);
                      });
}

int vcfc_ld_window_regions_file(vcfc_ctx *c, const char *in_path, const char *out_tsv, uint64_t window, double min_r2,
                                const uint8_t *table, uint64_t table_bytes) {
    if (!c || !in_path || !out_tsv || !vcfc_reg::regions_validate(table, table_bytes) || window == 0 ||
        window >= (1ull << 16))
        return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    const uint8_t *d_table = nullptr;
    const vcfc_dec::MatchStep match = vcfc_reg::regions_step(table, table_bytes, &d_table);
    return ld_to_file(c, in_path, out_tsv, window, min_r2,
                      [&](const uint8_t *p, uint64_t pn, vcfc_dec::Buffers &B, vcfc_ld::Result &R, uint64_t *data_off,
                          uint64_t *S) { return vcfc_ld::window_file(p, pn, window, &match, B, c->stream, R, data_off, S); });
}

// ---- kinship; driver in vcfc_kin_driver.h ------------------------

uint64_t vcfc_kin_workspace_size(uint64_t n_records, uint64_t samples) {
    return vcfc_kin_workspace_layout(n_records, samples).total;
}

int vcfc_kin_tables_device(const uint8_t *d_bed, uint64_t n_rows, uint64_t row_stride, uint64_t samples, uint32_t *d_tables,
                           uint64_t tables_cap, int accumulate, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream) {
    return vcfc_kin::tables_device(d_bed, n_rows, row_stride, samples, d_tables, tables_cap, accumulate, d_ws, ws_bytes, d_err,
                                   static_cast<hipStream_t>(stream));
}

int vcfc_kin_records_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start, const uint8_t *d_select,
                            uint64_t n, uint64_t samples, uint32_t *d_tables, uint64_t tables_cap, int accumulate,
                            uint64_t *d_row_of, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream) {
    return vcfc_kin::records_device(d_in, in_bytes, d_rec_start, d_select, n, samples, d_tables, tables_cap, accumulate, d_row_of,
                                    d_ws, ws_bytes, d_err, static_cast<hipStream_t>(stream));
}

namespace {
// run(in, n, B, R, &data_off, &S): the square of a .vcfc by one of the two match steps
using KinRun = std::function<int(const uint8_t *, uint64_t, vcfc_dec::Buffers &, vcfc_kin::Result &, uint64_t *, uint64_t *)>;

// what the two kinship buffer entries hand back
int kin_to_caller(vcfc_ctx *c, const uint8_t *in, uint64_t n, uint64_t *rec_index, uint64_t rows_cap, uint32_t *tables,
                  uint64_t tables_cap, uint64_t *n_rows, uint64_t *n_samples, uint64_t *err_record, const KinRun &run) {
    if (!c || (!in && n) || (!rec_index && rows_cap) || (!tables && tables_cap) || !n_rows || !n_samples || !err_record)
        return VCFC_E_ARG;
    *n_rows = *n_samples = 0;
    *err_record = ~0ull;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    vcfc_kin::Result R;
    uint64_t data_off = 0, S = 0;
    CtxDecodeBuffers B(c);
    const int st = run(in, n, B, R, &data_off, &S);
    if (st != VCFC_OK && st != VCFC_E_FORMAT) return st;
    *n_rows = R.index.size();
    *n_samples = S;
    *err_record = R.err_record;
    if (*n_rows > rows_cap || R.tables.size() / 9 > tables_cap) return VCFC_E_NOSPACE;
    if (*n_rows) memcpy(rec_index, R.index.data(), 8 * R.index.size());
    if (!R.tables.empty()) memcpy(tables, R.tables.data(), 4 * R.tables.size());
    return st;
}

// the text file of a kinship entry
int kin_to_file(vcfc_ctx *c, const char *in_path, const char *out_path, int has_min, double min_kinship, const KinRun &run) {
    const int fd = open(out_path, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fd < 0) return VCFC_E_IO;
    MappedFile f;
    int st = f.open_ro(in_path);
    if (!st) {
        vcfc_kin::Result R;
        uint64_t data_off = 0, S = 0;
        CtxDecodeBuffers B(c);
        st = run(f.p, f.n, B, R, &data_off, &S);
        if (data_off && S && !R.tables.empty() && (st == VCFC_OK || st == VCFC_E_FORMAT)) {   // past the header
            std::vector<uint8_t> text;
            vcfc_kin::render_tsv(f.p, data_off, S, R, has_min != 0, min_kinship, text);
            if (write_all_at(fd, text.data(), text.size(), 0)) st = VCFC_E_IO;
        }
    }
    if (close(fd) != 0 && !st) st = VCFC_E_IO;
    return st;
}
}  // namespace

int vcfc_kinship_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, int has_query, const char *ref, uint64_t ref_len,
                        int has_range, uint64_t start, uint64_t end, uint64_t *rec_index, uint64_t rows_cap, uint32_t *tables,
                        uint64_t tables_cap, uint64_t *n_rows, uint64_t *n_samples, uint64_t *err_record) {
    if (has_query && !ref && ref_len) return VCFC_E_ARG;
    const vcfc_kin::Query q{reinterpret_cast<const uint8_t *>(ref), ref_len, has_range, start, end};
    return kin_to_caller(c, in, n, rec_index, rows_cap, tables, tables_cap, n_rows, n_samples, err_record,
                         [&](const uint8_t *p, uint64_t pn, vcfc_dec::Buffers &B, vcfc_kin::Result &R, uint64_t *data_off,
                             uint64_t *S) { return vcfc_kin::kin_file(p, pn, has_query ? &q : nullptr, B, c->stream, R, data_off, S); });
}

int vcfc_kinship_regions_buffer(vcfc_ctx *c, const uint8_t *in, uint64_t n, const uint8_t *table, uint64_t table_bytes,
                                uint64_t *rec_index, uint64_t rows_cap, uint32_t *tables, uint64_t tables_cap, uint64_t *n_rows,
                                uint64_t *n_samples, uint64_t *err_record) {
    if (!vcfc_reg::regions_validate(table, table_bytes)) return VCFC_E_ARG;
    const uint8_t *d_table = nullptr;
    const vcfc_dec::MatchStep match = vcfc_reg::regions_step(table, table_bytes, &d_table);
    return kin_to_caller(c, in, n, rec_index, rows_cap, tables, tables_cap, n_rows, n_samples, err_record,
                         [&](const uint8_t *p, uint64_t pn, vcfc_dec::Buffers &B, vcfc_kin::Result &R, uint64_t *data_off,
                             uint64_t *S) { return vcfc_kin::kin_file(p, pn, &match, B, c->stream, R, data_off, S); });
}

int vcfc_kinship_file(vcfc_ctx *c, const char *in_path, const char *out_tsv, int has_min, double min_kinship, int has_query,
                      const char *ref, uint64_t ref_len, int has_range, uint64_t start, uint64_t end) {
    if (!c || !in_path || !out_tsv || (has_query && !ref && ref_len)) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    const vcfc_kin::Query q{reinterpret_cast<const uint8_t *>(ref), ref_len, has_range, start, end};
    return kin_to_file(c, in_path, out_tsv, has_min, min_kinship,
                       [&](const uint8_t *p, uint64_t pn, vcfc_dec::Buffers &B, vcfc_kin::Result &R, uint64_t *data_off,
                           uint64_t *S) { return vcfc_kin::kin_file(p, pn, has_query ? &q : nullptr, B, c->stream, R, data_off, S); });
}

int vcfc_kinship_regions_file(vcfc_ctx *c, const char *in_path, const char *out_tsv, int has_min, double min_kinship,
                              const uint8_t *table, uint64_t table_bytes) {
    if (!c || !in_path || !out_tsv || !vcfc_reg::regions_validate(table, table_bytes)) return VCFC_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return VCFC_E_HIP;
    const uint8_t *d_table = nullptr;
    const vcfc_dec::MatchStep match = vcfc_reg::regions_step(table, table_bytes, &d_table);
    return kin_to_file(c, in_path, out_tsv, has_min, min_kinship,
                       [&](const uint8_t *p, uint64_t pn, vcfc_dec::Buffers &B, vcfc_kin::Result &R, uint64_t *data_off,
                           uint64_t *S) { return vcfc_kin::kin_file(p, pn, &match, B, c->stream, R, data_off, S); });
}

int vcfc_query_match_device(const uint8_t *d_in, const uint64_t *d_rec_start, uint64_t n, const uint8_t *d_ref,
                            uint64_t ref_len, int has_range, uint64_t start, uint64_t end, uint8_t *d_flag,
                            uint64_t *d_err, void *stream) {
    if ((n && (!d_in || !d_rec_start || !d_flag)) || (!d_ref && ref_len) || ref_len > 0xFFFFFFFFull || !d_err)
        return VCFC_E_ARG;
    VcfcQuery q;
    q.ref = d_ref; q.ref_len = (uint32_t)ref_len; q.has_range = has_range ? 1u : 0u; q.start = start; q.end = end;
    return vcfc_query_match(d_in, d_rec_start, n, q, d_flag, d_err, static_cast<hipStream_t>(stream)) == hipSuccess
               ? VCFC_OK : VCFC_E_HIP;
}

int vcfc_record_hash_device(const uint8_t *d_recs, const uint64_t *d_rec_off, uint64_t n, uint64_t *d_hash,
                            void *stream) {
    if (n && (!d_recs || !d_rec_off || !d_hash)) return VCFC_E_ARG;
    return vcfc_record_hash(d_recs, d_rec_off, n, d_hash, static_cast<hipStream_t>(stream)) == hipSuccess
               ? VCFC_OK : VCFC_E_HIP;
}

uint64_t vcfc_decode_workspace_size(uint64_t n_records) { return vcfc_decode_workspace_layout(n_records).total; }

int vcfc_decode_selected_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start,
                                const uint8_t *d_select, uint64_t n, uint64_t samples, uint8_t *d_out, uint64_t out_cap,
                                uint64_t *d_line_off, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, int exact,
                                void *stream) {
    if ((n && (!d_in || !d_rec_start || !d_out || !d_ws)) || !d_line_off || !d_err) return VCFC_E_ARG;
    const VcfcDecodeLayout L = vcfc_decode_workspace_layout(n);
    if (ws_bytes < L.total) return VCFC_E_NOSPACE;
    uint8_t *ws = static_cast<uint8_t *>(d_ws);
    hipStream_t s = static_cast<hipStream_t>(stream);
    VcfcDecodeArgs a;
    a.in = d_in; a.n_bytes = in_bytes; a.rec_start = d_rec_start; a.select = d_select; a.n = n; a.S = samples;
    a.out = d_out; a.out_cap = out_cap; a.line_off = d_line_off;
    a.st = reinterpret_cast<uint32_t *>(ws + L.st);
    a.line_size = reinterpret_cast<uint32_t *>(ws + L.line_size);
    a.end = reinterpret_cast<uint64_t *>(ws + L.end);
    a.seq_list = reinterpret_cast<uint32_t *>(ws + L.seq_list);
    a.seq_count = reinterpret_cast<uint32_t *>(ws + L.seq_count);
    a.err = d_err;
    a.partials = reinterpret_cast<uint64_t *>(ws + L.partials);
    if (vcfc_decode_plan(a, exact != 0, s) != hipSuccess) return VCFC_E_HIP;
    return vcfc_decode_write(a, 0, n, s) == hipSuccess ? VCFC_OK : VCFC_E_HIP;
}

int vcfc_decode_records_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start, uint64_t n,
                               uint64_t samples, uint8_t *d_out, uint64_t out_cap, uint64_t *d_line_off, void *d_ws,
                               uint64_t ws_bytes, uint64_t *d_err, int exact, void *stream) {
    return vcfc_decode_selected_device(d_in, in_bytes, d_rec_start, nullptr, n, samples, d_out, out_cap, d_line_off,
                                       d_ws, ws_bytes, d_err, exact, stream);
}

}  // extern "C"
