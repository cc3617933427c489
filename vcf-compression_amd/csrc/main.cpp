// main.cpp -- CLI with the reference's argv contract (src/main.cpp:4028-4185)
// for the codec path: `main compress|decompress|sparsify <in> <out>` and
// `main query|sparse-query <in> <query>`, and for the binned external index:
// `main create-binned-index <bin-size> <in>` and
// `main query-binned-index <in> <region>`, for the sparse external index:
// `main create-sparse-index <in>` and `main query-sparse-index <in> <region>`,
// and `main gap-analysis <in>`; beyond the reference, the sample subset:
// `main decompress-samples <in> <out> <names>` and
// `main query-samples <in> <query> <names>`, and the counts:
// `main genotype-counts <in> <variants.tsv> <samples.tsv> [<query>]`
// (DESIGN.md §4j), and the region lists: `main query-regions <in> <regions>`,
// `main query-samples-regions <in> <regions> <names>` and
// `main genotype-counts-regions <in> <variants.tsv> <samples.tsv> <regions>`
// (DESIGN.md §4k), and the PLINK 1 export: `main export-bed <in> <prefix>
// [<query>]` and `main export-bed-regions <in> <prefix> <regions>`, and the
// compressed-to-compressed cut: `main extract-samples <in>
// <out> <names> [<query>]` and `main extract-regions <in> <out> <regions>
// [<names>]`, and the pairwise LD of nearby rows: `main
// ld-window <in> <out.tsv> <window> <min-r2> [<query>]` and `main
// ld-window-regions <in> <out.tsv> <window> <min-r2> <regions>`, and the
// pairwise tables, IBS and kinship of the samples: `main
// kinship <in> <out.tsv> <min-kinship|all> [<query>]` and `main
// kinship-regions <in> <out.tsv> <min-kinship|all> <regions>`.  Data lines are
// encoded on the GPU through libvcfc.so.  Error messages mirror the
// reference's exceptions (which terminate the reference process).
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "vcfc.h"

static int usage() {
    fprintf(stderr, "./main [compress|decompress|sparsify] <input_file> <output_file>\n"
                    "./main [query|sparse-query] <input_file> <ref>[:<start>-<end>]\n"
                    "./main create-binned-index <bin-size> <compressed-filename>\n"
                    "./main query-binned-index <compressed-filename> <region>\n"
                    "./main create-sparse-index <compressed-filename>\n"
                    "./main query-sparse-index <compressed-filename> <region>\n"
                    "./main gap-analysis <compressed-filename>\n"
                    "./main decompress-samples <input_file> <output_file> <name>[,<name>...]\n"
                    "./main query-samples <input_file> <ref>[:<start>-<end>] <name>[,<name>...]\n"
                    "./main genotype-counts <input_file> <variants.tsv> <samples.tsv> [<ref>[:<start>-<end>]]\n"
                    "./main query-regions <input_file> <regions-file>\n"
                    "./main query-samples-regions <input_file> <regions-file> <name>[,<name>...]\n"
                    "./main genotype-counts-regions <input_file> <variants.tsv> <samples.tsv> <regions-file>\n"
                    "./main export-bed <input_file> <output_prefix> [<ref>[:<start>-<end>]]\n"
                    "./main export-bed-regions <input_file> <output_prefix> <regions-file>\n"
                    "./main extract-samples <input_file> <output_file> <name>[,<name>...] [<ref>[:<start>-<end>]]\n"
                    "./main extract-regions <input_file> <output_file> <regions-file> [<name>[,<name>...]]\n"
                    "./main ld-window <input_file> <out.tsv> <window> <min-r2> [<ref>[:<start>-<end>]]\n"
                    "./main ld-window-regions <input_file> <out.tsv> <window> <min-r2> <regions-file>\n"
                    "./main kinship <input_file> <out.tsv> <min-kinship|all> [<ref>[:<start>-<end>]]\n"
                    "./main kinship-regions <input_file> <out.tsv> <min-kinship|all> <regions-file>\n");
    return 1;
}

// The sample columns of a comma-separated name list, resolved against the
// header of `path` (read as a growing prefix of the file).  0: cols filled;
// 1: a message was printed (unknown / duplicate name); VCFC_E_FORMAT /
// VCFC_E_IO otherwise.
static int resolve_samples(const char *path, const std::string &names, std::vector<uint32_t> &cols) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return VCFC_E_IO;
    struct stat sb;
    if (fstat(fd, &sb) != 0) { close(fd); return VCFC_E_IO; }
    const uint64_t fsize = (uint64_t)sb.st_size;
    std::vector<uint8_t> buf;
    cols.resize(names.size() + 1);
    int st = VCFC_E_FORMAT;
    uint64_t n_cols = 0, bad = 0;
    for (uint64_t want = 1ull << 20;; want *= 4) {
        buf.resize(std::min<uint64_t>(want, fsize));
        uint64_t got = 0;
        while (got < buf.size()) {
            const ssize_t r = pread(fd, buf.data() + got, buf.size() - got, (off_t)got);
            if (r <= 0) break;
            got += (uint64_t)r;
        }
        st = vcfc_sample_columns(buf.data(), got, names.data(), names.size(), cols.data(), cols.size(), &n_cols, &bad);
        if (st != VCFC_E_FORMAT || buf.size() >= fsize) break;   // (a header cut short does not parse: read more)
    }
    close(fd);
    if (st == VCFC_E_ARG) {
        const size_t e = names.find(',', bad);
        const std::string name = names.substr(bad, e == std::string::npos ? e : e - bad);
        // every name before this one resolved: listed there too, it is a duplicate
        const bool dup = ("," + names.substr(0, bad)).find("," + name + ",") != std::string::npos;
        printf("%s sample name: %s\n", dup ? "Duplicate" : "Unknown", name.c_str());
        return 1;
    }
    cols.resize(st == VCFC_OK ? n_cols : 0);
    return st;
}

// The region table of a regions file (BED or <ref>[:<start>-<end>] lines).
// 0: table filled; 1: a message was printed (the file cannot be read, or a
// line does not parse).
static int load_regions(const char *path, std::vector<uint8_t> &table) {
    std::string text;
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "Cannot read regions file: %s\n", path);
        return 1;
    }
    char buf[1 << 16];
    size_t r;
    while ((r = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, r);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) {
        fprintf(stderr, "Cannot read regions file: %s\n", path);
        return 1;
    }
    uint64_t bytes = 0, n_regions = 0, bad_line = 0;
    int st = vcfc_regions_build(text.data(), text.size(), nullptr, 0, &bytes, &n_regions, &bad_line);
    if (st == VCFC_E_NOSPACE) {
        table.resize(bytes);
        st = vcfc_regions_build(text.data(), text.size(), table.data(), table.size(), &bytes, &n_regions, &bad_line);
    }
    if (st == VCFC_E_ARG && bad_line) {
        size_t a = 0;
        for (uint64_t l = 1; l < bad_line; l++) a = text.find('\n', a) + 1;
        size_t e = text.find('\n', a);
        if (e == std::string::npos) e = text.size();
        else if (e > a && text[e - 1] == '\r') e--;
        printf("Failed to parse region at line %llu: %s\n", (unsigned long long)bad_line, text.substr(a, e - a).c_str());
        return 1;
    }
    if (st != VCFC_OK) {
        fprintf(stderr, "Cannot build the region table: %s\n", vcfc_strerror(st));
        return 1;
    }
    return 0;
}

static bool file_exists(const char *p) {
    struct stat s;
    return stat(p, &s) == 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return usage();
    std::string action(argv[1]);
    if (action == "compress") {
        if (argc < 4) return usage();
        const bool exists = file_exists(argv[2]);
        if (!exists) printf("Input file does not exist: %s\n", argv[2]);
        if (std::string(argv[2]) == argv[3]) {
            fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                            "  what():  input and output file are the same\n");
            return 134;
        }
        if (!exists) {   // the reference's ifstream reads nothing: an empty output, exit 0
            FILE *f = fopen(argv[3], "w");
            if (f) fclose(f);
            return 0;
        }
        vcfc_ctx *ctx = nullptr;
        int st = vcfc_ctx_create(0, &ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
            return 1;
        }
        int64_t err_line = -1;
        st = vcfc_compress_file(ctx, argv[2], argv[3], &err_line);
        vcfc_ctx_destroy(ctx);
        if (st == VCFC_E_LT8COLS || st == VCFC_E_HEADER) {
            fprintf(stderr, "terminate called after throwing an instance of 'VcfValidationError'\n"
                            "  what():  %s (input line %lld)\n", vcfc_strerror(st), (long long)err_line);
            return 134;
        }
        if (st == VCFC_E_8COLS) {
            fprintf(stderr, "terminate called after throwing an instance of 'std::length_error'\n"
                            "  what():  vector::_M_default_append (input line %lld)\n", (long long)err_line);
            return 134;
        }
        if (st != VCFC_OK) {
            fprintf(stderr, "Error in compression of file: %s\n", vcfc_strerror(st));
            return 1;
        }
        return 0;
    }
    if (action == "decompress") {
        // src/main.cpp:4038-4056 -> decompress2_fd (src/compress.cpp:1214)
        if (argc < 4) return usage();
        if (!file_exists(argv[2])) printf("Input file does not exist: %s\n", argv[2]);
        if (std::string(argv[2]) == argv[3]) {
            fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                            "  what():  input and output file are the same\n");
            return 134;
        }
        vcfc_ctx *ctx = nullptr;
        int st = vcfc_ctx_create(0, &ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
            return 1;
        }
        st = vcfc_decompress_file(ctx, argv[2], argv[3]);
        vcfc_ctx_destroy(ctx);
        if (st == VCFC_E_FORMAT) {
            fprintf(stderr, "terminate called after throwing an instance of 'VcfValidationError'\n"
                            "  what():  %s\n", vcfc_strerror(st));
            return 134;
        }
        if (st != VCFC_OK) {
            fprintf(stderr, "Error in compression of file: %s\n", vcfc_strerror(st));
            return 1;
        }
        return 0;
    }
    if (action == "sparsify") {
        // src/main.cpp:4073-4085
        if (argc < 4) return usage();
        if (std::string(argv[2]) == argv[3]) {
            fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                            "  what():  input and output file are the same\n");
            return 134;
        }
        if (!file_exists(argv[2])) printf("Input file does not exist: %s\n", argv[2]);
        vcfc_ctx *ctx = nullptr;
        int st = vcfc_ctx_create(0, &ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
            return 1;
        }
        st = vcfc_sparsify_file(ctx, argv[2], argv[3]);
        vcfc_ctx_destroy(ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "terminate called after throwing an instance of 'VcfValidationError'\n"
                            "  what():  %s\n", vcfc_strerror(st));
            return 134;
        }
        return 0;
    }
    if (action == "query" || action == "sparse-query") {
        // src/main.cpp:4057-4069 -> parse_coordinate_string (:3993-4026),
        // query_compressed_file (:3777-3929); src/main.cpp:4086-4096 ->
        // query_sparse_file_fd (:235-582).  Matching lines go to stdout.
        const bool sparse = action == "sparse-query";
        if (argc < 4) return usage();
        if (!sparse && !file_exists(argv[2])) printf("Input file does not exist: %s\n", argv[2]);
        const std::string q(argv[3]);
        uint64_t ref_len = 0, start = 0, end = 0;
        int has_range = 0;
        const int pq = vcfc_parse_query(q.data(), q.size(), &ref_len, &has_range, &start, &end);
        if (pq != 0) {
            const size_t colon = q.find(':'), dash = q.find('-', colon + 1);
            if (pq == 1) printf("Query must contain a dash character: <ref>:<start>-<end>\n");
            else if (pq == 2) printf("Failed to parse int from start position: %s\n", q.substr(colon + 1, dash - colon - 1).c_str());
            else printf("Failed to parse int from end position: %s\n", q.substr(dash + 1).c_str());
            printf("Failed to parse query string: %s\n", q.c_str());
            return 1;
        }
        vcfc_ctx *ctx = nullptr;
        int st = vcfc_ctx_create(0, &ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
            return 1;
        }
        fflush(stdout);
        st = sparse ? vcfc_sparse_query_file(ctx, argv[2], q.data(), ref_len, has_range, start, end, 1)
                    : vcfc_query_file(ctx, argv[2], q.data(), ref_len, has_range, start, end, 1);
        vcfc_ctx_destroy(ctx);
        if (st == VCFC_E_IO && sparse) {
            perror("open");
            fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                            "  what():  Failed to open file: %s\n", argv[2]);
            return 134;
        }
        if (st != VCFC_OK) {
            fprintf(stderr, "terminate called after throwing an instance of 'VcfValidationError'\n"
                            "  what():  %s\n", vcfc_strerror(st));
            return 134;
        }
        return 0;
    }
    if (action == "create-binned-index") {
        // src/main.cpp:4097-4115 -> create_binned_index4 (:1284-1637): writes <file>.vcfci
        if (argc != 4) {
            printf("Usage: ./main create-binned-index <bin-size> <compressed-filename>\n");
            return 1;
        }
        char *endp = nullptr;
        const unsigned long bin = strtoul(argv[2], &endp, 10);   // str_to_uint64 (src/utils.cpp:152-165)
        if (endp != argv[2] + strlen(argv[2]) || bin == 0) {     // (0: the reference dies of SIGFPE)
            printf("bin size must be a positive integer\n");
            return 1;
        }
        const std::string index = std::string(argv[3]) + ".vcfci";
        if (!file_exists(argv[3])) {
            perror("fopen");
            fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                            "  what():  Failed to open file: %s\n", argv[3]);
            return 134;
        }
        vcfc_ctx *ctx = nullptr;
        int st = vcfc_ctx_create(0, &ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
            return 1;
        }
        st = vcfc_create_binned_index_file(ctx, argv[3], index.c_str(), bin);
        vcfc_ctx_destroy(ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                            "  what():  %s\n", vcfc_strerror(st));
            return 134;
        }
        return 0;
    }
    if (action == "query-binned-index") {
        // src/main.cpp:4117-4143 -> query_binned_index_binarysearch (:2974-3349)
        if (argc < 4) {
            printf("Usage: ./main query-binned-index <compressed-filename> <region>");
            return 1;
        }
        const std::string index = std::string(argv[2]) + ".vcfci";
        if (!file_exists(argv[2])) {
            printf("Input file does not exist: %s\n", argv[2]);
            return 1;
        }
        if (!file_exists(index.c_str())) {
            printf("Index file does not exist: %s\n", index.c_str());
            return 1;
        }
        const std::string q(argv[3]);
        uint64_t ref_len = 0, start = 0, end = 0;
        int has_range = 0;
        const int pq = vcfc_parse_query(q.data(), q.size(), &ref_len, &has_range, &start, &end);
        if (pq != 0) {
            const size_t colon = q.find(':'), dash = q.find('-', colon + 1);
            if (pq == 1) printf("Query must contain a dash character: <ref>:<start>-<end>\n");
            else if (pq == 2) printf("Failed to parse int from start position: %s\n", q.substr(colon + 1, dash - colon - 1).c_str());
            else printf("Failed to parse int from end position: %s\n", q.substr(dash + 1).c_str());
            printf("Failed to parse query string: %s\n", q.c_str());
            return 1;
        }
        vcfc_ctx *ctx = nullptr;
        int st = vcfc_ctx_create(0, &ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
            return 1;
        }
        fflush(stdout);
        st = vcfc_query_binned_index_file(ctx, argv[2], index.c_str(), q.data(), ref_len, has_range, start, end, 1);
        vcfc_ctx_destroy(ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                            "  what():  %s\n", vcfc_strerror(st));
            return 134;
        }
        return 0;
    }
    if (action == "create-sparse-index") {
        // src/main.cpp:4144-4157 -> create_sparse_external_index (:854-999): writes <file>.vcfci-sparse
        if (argc != 3) {
            printf("Usage: ./main create-sparse-index <compressed-filename>\n");
            return 1;
        }
        const std::string index = std::string(argv[2]) + ".vcfci-sparse";
        if (!file_exists(argv[2])) {   // thrown before the index is created (:858-862)
            perror("fopen");
            fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                            "  what():  Failed to open file: %s\n", argv[2]);
            return 134;
        }
        vcfc_ctx *ctx = nullptr;
        int st = vcfc_ctx_create(0, &ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
            return 1;
        }
        int64_t err_record = -1;
        int seek_failed = 0;
        st = vcfc_create_sparse_index_file(ctx, argv[2], index.c_str(), &err_record, &seek_failed);
        vcfc_ctx_destroy(ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                            "  what():  %s (record %lld)\n", vcfc_strerror(st), (long long)err_record);
            return 134;
        }
        if (seek_failed) fprintf(stderr, "lseek: Invalid argument\n");   // perror("lseek"), then return (:954-959)
        return 0;
    }
    if (action == "query-sparse-index") {
        // src/main.cpp:4158-4177 -> query_sparse_external_index (:1002-1281)
        if (argc != 4) {
            printf("Usage: ./main query-sparse-index <compressed-filename> <region>\n");
            return 1;
        }
        const std::string index = std::string(argv[2]) + ".vcfci-sparse";
        const std::string q(argv[3]);
        uint64_t ref_len = 0, start = 0, end = 0;
        int has_range = 0;
        const int pq = vcfc_parse_query(q.data(), q.size(), &ref_len, &has_range, &start, &end);
        if (pq != 0) {
            const size_t colon = q.find(':'), dash = q.find('-', colon + 1);
            if (pq == 1) printf("Query must contain a dash character: <ref>:<start>-<end>\n");
            else if (pq == 2) printf("Failed to parse int from start position: %s\n", q.substr(colon + 1, dash - colon - 1).c_str());
            else printf("Failed to parse int from end position: %s\n", q.substr(dash + 1).c_str());
            printf("Failed to parse query string: %s\n", q.c_str());
            return 1;
        }
        // the reference's early returns, each with exit 0 (:1019-1047, :1077-1082)
        if (!file_exists(argv[2])) {
            errno = ENOENT;
            perror("fopen");
            return 0;
        }
        if (!file_exists(index.c_str())) return 0;
        {
            const int ifd = open(index.c_str(), O_RDONLY);
            if (ifd < 0) {
                perror("open");
                return 0;
            }
            const off_t probe = lseek(ifd, 10000000, SEEK_DATA);
            if (probe < 0) perror("fseek");   // (the reference's label)
            close(ifd);
            if (probe < 0) return 0;
        }
        if ((int64_t)vcfc_sparse_index_offset(has_range ? start : 0) < 0) {
            errno = EINVAL;
            perror("lseek");
            return 0;
        }
        vcfc_ctx *ctx = nullptr;
        int st = vcfc_ctx_create(0, &ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
            return 1;
        }
        fflush(stdout);
        st = vcfc_query_sparse_index_file(ctx, argv[2], index.c_str(), q.data(), ref_len, has_range, start, end, 1);
        vcfc_ctx_destroy(ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "terminate called after throwing an instance of 'VcfValidationError'\n"
                            "  what():  %s\n", vcfc_strerror(st));
            return 134;
        }
        return 0;
    }
    if (action == "gap-analysis") {
        // src/main.cpp:4035-4037 -> gap_analysis (:3931-3980): writes start-positions.txt in the
        // current directory.  Without a file name the reference dies in std::string(nullptr); here: usage.
        if (argc < 3) return usage();
        if (!file_exists(argv[2])) {   // the reference reads from fd -1 and throws on the empty header
            fprintf(stderr, "terminate called after throwing an instance of 'VcfValidationError'\n"
                            "  what():  Failed to open file: %s\n", argv[2]);
            return 134;
        }
        vcfc_ctx *ctx = nullptr;
        int st = vcfc_ctx_create(0, &ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
            return 1;
        }
        st = vcfc_gap_analysis_file(ctx, argv[2], "start-positions.txt");
        vcfc_ctx_destroy(ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "terminate called after throwing an instance of 'VcfValidationError'\n"
                            "  what():  %s\n", vcfc_strerror(st));
            return 134;
        }
        return 0;
    }
    if (action == "decompress-samples" || action == "query-samples") {
        // no reference counterpart: the chosen samples' columns of `decompress` / `query`
        const bool query = action == "query-samples";
        if (argc < 5) return usage();
        if (!file_exists(argv[2])) printf("Input file does not exist: %s\n", argv[2]);
        if (!query && std::string(argv[2]) == argv[3]) {
            fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                            "  what():  input and output file are the same\n");
            return 134;
        }
        const std::string q(query ? argv[3] : "");
        uint64_t ref_len = 0, start = 0, end = 0;
        int has_range = 0;
        if (query) {
            const int pq = vcfc_parse_query(q.data(), q.size(), &ref_len, &has_range, &start, &end);
            if (pq != 0) {
                const size_t colon = q.find(':'), dash = q.find('-', colon + 1);
                if (pq == 1) printf("Query must contain a dash character: <ref>:<start>-<end>\n");
                else if (pq == 2) printf("Failed to parse int from start position: %s\n", q.substr(colon + 1, dash - colon - 1).c_str());
                else printf("Failed to parse int from end position: %s\n", q.substr(dash + 1).c_str());
                printf("Failed to parse query string: %s\n", q.c_str());
                return 1;
            }
        }
        std::vector<uint32_t> cols;
        int st = resolve_samples(argv[2], argv[4], cols);
        if (st == 1) return 1;   // unknown / duplicate name: message printed, nothing written
        if (st == VCFC_OK) {
            vcfc_ctx *ctx = nullptr;
            st = vcfc_ctx_create(0, &ctx);
            if (st != VCFC_OK) {
                fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
                return 1;
            }
            fflush(stdout);
            st = query ? vcfc_query_samples_file(ctx, argv[2], q.data(), ref_len, has_range, start, end, cols.data(),
                                                 cols.size(), 1)
                       : vcfc_decompress_samples_file(ctx, argv[2], argv[3], cols.data(), cols.size());
            vcfc_ctx_destroy(ctx);
        }
        if (st == VCFC_E_FORMAT) {
            fprintf(stderr, "terminate called after throwing an instance of 'VcfValidationError'\n"
                            "  what():  %s\n", vcfc_strerror(st));
            return 134;
        }
        if (st != VCFC_OK) {
            fprintf(stderr, "Error in decompression of file: %s\n", vcfc_strerror(st));
            return 1;
        }
        return 0;
    }
    if (action == "genotype-counts") {
        // no reference counterpart: per-variant and per-sample genotype counts as two TSV files
        if (argc < 5) return usage();
        if (!file_exists(argv[2])) printf("Input file does not exist: %s\n", argv[2]);
        if (std::string(argv[2]) == argv[3] || std::string(argv[2]) == argv[4] || std::string(argv[3]) == argv[4]) {
            fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                            "  what():  input and output file are the same\n");
            return 134;
        }
        const bool query = argc > 5;
        const std::string q(query ? argv[5] : "");
        uint64_t ref_len = 0, start = 0, end = 0;
        int has_range = 0;
        if (query) {
            const int pq = vcfc_parse_query(q.data(), q.size(), &ref_len, &has_range, &start, &end);
            if (pq != 0) {
                const size_t colon = q.find(':'), dash = q.find('-', colon + 1);
                if (pq == 1) printf("Query must contain a dash character: <ref>:<start>-<end>\n");
                else if (pq == 2) printf("Failed to parse int from start position: %s\n", q.substr(colon + 1, dash - colon - 1).c_str());
                else printf("Failed to parse int from end position: %s\n", q.substr(dash + 1).c_str());
                printf("Failed to parse query string: %s\n", q.c_str());
                return 1;
            }
        }
        vcfc_ctx *ctx = nullptr;
        int st = vcfc_ctx_create(0, &ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
            return 1;
        }
        fflush(stdout);
        st = vcfc_genotype_counts_file(ctx, argv[2], argv[3], argv[4], query ? 1 : 0, q.data(), ref_len, has_range, start, end);
        vcfc_ctx_destroy(ctx);
        if (st == VCFC_E_FORMAT) {
            fprintf(stderr, "terminate called after throwing an instance of 'VcfValidationError'\n"
                            "  what():  %s\n", vcfc_strerror(st));
            return 134;
        }
        if (st != VCFC_OK) {
            fprintf(stderr, "Error in genotype-counts of file: %s\n", vcfc_strerror(st));
            return 1;
        }
        return 0;
    }
    if (action == "query-regions" || action == "query-samples-regions" || action == "genotype-counts-regions") {
        // no reference counterpart: `query`, `query-samples` and `genotype-counts` over a region list
        const bool samples = action == "query-samples-regions", counts = action == "genotype-counts-regions";
        if (argc < (counts ? 6 : samples ? 5 : 4)) return usage();
        std::vector<uint8_t> table;
        if (load_regions(argv[counts ? 5 : 3], table)) return 1;   // before the input is opened
        if (!file_exists(argv[2])) printf("Input file does not exist: %s\n", argv[2]);
        if (counts && (std::string(argv[2]) == argv[3] || std::string(argv[2]) == argv[4] || std::string(argv[3]) == argv[4])) {
            fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                            "  what():  input and output file are the same\n");
            return 134;
        }
        std::vector<uint32_t> cols;
        int st = samples ? resolve_samples(argv[2], argv[4], cols) : VCFC_OK;
        if (st == 1) return 1;   // unknown / duplicate name: message printed, nothing written
        if (st == VCFC_OK) {
            vcfc_ctx *ctx = nullptr;
            st = vcfc_ctx_create(0, &ctx);
            if (st != VCFC_OK) {
                fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
                return 1;
            }
            fflush(stdout);
            if (counts) st = vcfc_genotype_counts_regions_file(ctx, argv[2], argv[3], argv[4], table.data(), table.size());
            else if (samples) st = vcfc_query_samples_regions_file(ctx, argv[2], table.data(), table.size(), cols.data(), cols.size(), 1);
            else st = vcfc_query_regions_file(ctx, argv[2], table.data(), table.size(), 1);
            vcfc_ctx_destroy(ctx);
        }
        if (st == VCFC_E_FORMAT) {
            fprintf(stderr, "terminate called after throwing an instance of 'VcfValidationError'\n"
                            "  what():  %s\n", vcfc_strerror(st));
            return 134;
        }
        if (st != VCFC_OK) {
            fprintf(stderr, "Error in %s of file: %s\n", counts ? "genotype-counts" : "decompression", vcfc_strerror(st));
            return 1;
        }
        return 0;
    }
    if (action == "export-bed" || action == "export-bed-regions") {
        // no reference counterpart: the genotype matrix as PLINK 1 <prefix>.bed / .bim / .fam
        const bool regions = action == "export-bed-regions";
        if (argc < (regions ? 5 : 4)) return usage();
        std::vector<uint8_t> table;
        if (regions && load_regions(argv[4], table)) return 1;   // before the input is opened
        if (!file_exists(argv[2])) printf("Input file does not exist: %s\n", argv[2]);
        for (const char *ext : {".bed", ".bim", ".fam"})
            if (std::string(argv[3]) + ext == argv[2]) {
                fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                                "  what():  input and output file are the same\n");
                return 134;
            }
        const bool query = !regions && argc > 4;
        const std::string q(query ? argv[4] : "");
        uint64_t ref_len = 0, start = 0, end = 0;
        int has_range = 0;
        if (query) {
            const int pq = vcfc_parse_query(q.data(), q.size(), &ref_len, &has_range, &start, &end);
            if (pq != 0) {
                const size_t colon = q.find(':'), dash = q.find('-', colon + 1);
                if (pq == 1) printf("Query must contain a dash character: <ref>:<start>-<end>\n");
                else if (pq == 2) printf("Failed to parse int from start position: %s\n", q.substr(colon + 1, dash - colon - 1).c_str());
                else printf("Failed to parse int from end position: %s\n", q.substr(dash + 1).c_str());
                printf("Failed to parse query string: %s\n", q.c_str());
                return 1;
            }
        }
        vcfc_ctx *ctx = nullptr;
        int st = vcfc_ctx_create(0, &ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
            return 1;
        }
        fflush(stdout);
        if (regions) st = vcfc_export_bed_regions_file(ctx, argv[2], argv[3], table.data(), table.size());
        else st = vcfc_export_bed_file(ctx, argv[2], argv[3], query ? 1 : 0, q.data(), ref_len, has_range, start, end);
        vcfc_ctx_destroy(ctx);
        if (st == VCFC_E_FORMAT) {
            fprintf(stderr, "terminate called after throwing an instance of 'VcfValidationError'\n"
                            "  what():  %s\n", vcfc_strerror(st));
            return 134;
        }
        if (st != VCFC_OK) {
            fprintf(stderr, "Error in export-bed of file: %s\n", vcfc_strerror(st));
            return 1;
        }
        return 0;
    }
    if (action == "extract-samples" || action == "extract-regions") {
        // no reference counterpart: a sample / region subset of a .vcfc, written as a .vcfc
        const bool regions = action == "extract-regions";
        if (argc < 5) return usage();
        std::vector<uint8_t> table;
        if (regions && load_regions(argv[4], table)) return 1;   // before the input is opened
        if (!file_exists(argv[2])) printf("Input file does not exist: %s\n", argv[2]);
        if (std::string(argv[2]) == argv[3]) {
            fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                            "  what():  input and output file are the same\n");
            return 134;
        }
        const bool query = !regions && argc > 5;
        const std::string q(query ? argv[5] : "");
        uint64_t ref_len = 0, start = 0, end = 0;
        int has_range = 0;
        if (query) {
            const int pq = vcfc_parse_query(q.data(), q.size(), &ref_len, &has_range, &start, &end);
            if (pq != 0) {
                const size_t colon = q.find(':'), dash = q.find('-', colon + 1);
                if (pq == 1) printf("Query must contain a dash character: <ref>:<start>-<end>\n");
                else if (pq == 2) printf("Failed to parse int from start position: %s\n", q.substr(colon + 1, dash - colon - 1).c_str());
                else printf("Failed to parse int from end position: %s\n", q.substr(dash + 1).c_str());
                printf("Failed to parse query string: %s\n", q.c_str());
                return 1;
            }
        }
        const bool named = !regions || argc > 5;   // extract-regions without names: all columns
        std::vector<uint32_t> cols;
        int st = named ? resolve_samples(argv[2], argv[regions ? 5 : 4], cols) : VCFC_OK;
        if (st == 1) return 1;   // unknown / duplicate name: message printed, nothing written
        if (st == VCFC_OK) {
            vcfc_ctx *ctx = nullptr;
            st = vcfc_ctx_create(0, &ctx);
            if (st != VCFC_OK) {
                fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
                return 1;
            }
            fflush(stdout);
            const uint32_t *cp = named ? cols.data() : nullptr;
            if (regions) st = vcfc_extract_regions_file(ctx, argv[2], argv[3], cp, cols.size(), table.data(), table.size());
            else st = vcfc_extract_file(ctx, argv[2], argv[3], cp, cols.size(), query ? 1 : 0, q.data(), ref_len, has_range, start, end);
            vcfc_ctx_destroy(ctx);
        }
        if (st == VCFC_E_FORMAT) {
            fprintf(stderr, "terminate called after throwing an instance of 'VcfValidationError'\n"
                            "  what():  %s\n", vcfc_strerror(st));
            return 134;
        }
        if (st != VCFC_OK) {
            fprintf(stderr, "Error in extract of file: %s\n", vcfc_strerror(st));
            return 1;
        }
        return 0;
    }
    if (action == "ld-window" || action == "ld-window-regions") {
        // no reference counterpart: genotype tables and r2 of the pairs of rows at most <window> apart
        const bool regions = action == "ld-window-regions";
        if (argc < (regions ? 7 : 6)) return usage();
        char *we = nullptr, *re = nullptr;
        errno = 0;
        const unsigned long long window = strtoull(argv[4], &we, 10);
        const double min_r2 = strtod(argv[5], &re);
        if (errno || !*argv[4] || *we || argv[4][0] == '-' || !*argv[5] || *re || window == 0 || window >= (1ull << 16)) return usage();
        std::vector<uint8_t> table;
        if (regions && load_regions(argv[6], table)) return 1;   // before the input is opened
        if (!file_exists(argv[2])) printf("Input file does not exist: %s\n", argv[2]);
        if (std::string(argv[2]) == argv[3]) {
            fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                            "  what():  input and output file are the same\n");
            return 134;
        }
        const bool query = !regions && argc > 6;
        const std::string q(query ? argv[6] : "");
        uint64_t ref_len = 0, start = 0, end = 0;
        int has_range = 0;
        if (query) {
            const int pq = vcfc_parse_query(q.data(), q.size(), &ref_len, &has_range, &start, &end);
            if (pq != 0) {
                const size_t colon = q.find(':'), dash = q.find('-', colon + 1);
                if (pq == 1) printf("Query must contain a dash character: <ref>:<start>-<end>\n");
                else if (pq == 2) printf("Failed to parse int from start position: %s\n", q.substr(colon + 1, dash - colon - 1).c_str());
                else printf("Failed to parse int from end position: %s\n", q.substr(dash + 1).c_str());
                printf("Failed to parse query string: %s\n", q.c_str());
                return 1;
            }
        }
        vcfc_ctx *ctx = nullptr;
        int st = vcfc_ctx_create(0, &ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
            return 1;
        }
        fflush(stdout);
        if (regions) st = vcfc_ld_window_regions_file(ctx, argv[2], argv[3], window, min_r2, table.data(), table.size());
        else st = vcfc_ld_window_file(ctx, argv[2], argv[3], window, min_r2, query ? 1 : 0, q.data(), ref_len, has_range, start, end);
        vcfc_ctx_destroy(ctx);
        if (st == VCFC_E_FORMAT) {
            fprintf(stderr, "terminate called after throwing an instance of 'VcfValidationError'\n"
                            "  what():  %s\n", vcfc_strerror(st));
            return 134;
        }
        if (st != VCFC_OK) {
            fprintf(stderr, "Error in ld-window of file: %s\n", vcfc_strerror(st));
            return 1;
        }
        return 0;
    }
    if (action == "kinship" || action == "kinship-regions") {
        // no reference counterpart: genotype tables, IBS and KING kinship of every pair of samples
        const bool regions = action == "kinship-regions";
        if (argc < (regions ? 6 : 5)) return usage();
        const bool all = std::string(argv[4]) == "all";
        char *re = nullptr;
        errno = 0;
        const double min_kinship = all ? 0.0 : strtod(argv[4], &re);
        if (!all && (errno || !*argv[4] || *re || min_kinship != min_kinship)) return usage();
        std::vector<uint8_t> table;
        if (regions && load_regions(argv[5], table)) return 1;   // before the input is opened
        if (!file_exists(argv[2])) printf("Input file does not exist: %s\n", argv[2]);
        if (std::string(argv[2]) == argv[3]) {
            fprintf(stderr, "terminate called after throwing an instance of 'std::runtime_error'\n"
                            "  what():  input and output file are the same\n");
            return 134;
        }
        const bool query = !regions && argc > 5;
        const std::string q(query ? argv[5] : "");
        uint64_t ref_len = 0, start = 0, end = 0;
        int has_range = 0;
        if (query) {
            const int pq = vcfc_parse_query(q.data(), q.size(), &ref_len, &has_range, &start, &end);
            if (pq != 0) {
                const size_t colon = q.find(':'), dash = q.find('-', colon + 1);
                if (pq == 1) printf("Query must contain a dash character: <ref>:<start>-<end>\n");
                else if (pq == 2) printf("Failed to parse int from start position: %s\n", q.substr(colon + 1, dash - colon - 1).c_str());
                else printf("Failed to parse int from end position: %s\n", q.substr(dash + 1).c_str());
                printf("Failed to parse query string: %s\n", q.c_str());
                return 1;
            }
        }
        vcfc_ctx *ctx = nullptr;
        int st = vcfc_ctx_create(0, &ctx);
        if (st != VCFC_OK) {
            fprintf(stderr, "vcfc: %s\n", vcfc_strerror(st));
            return 1;
        }
        fflush(stdout);
        if (regions) st = vcfc_kinship_regions_file(ctx, argv[2], argv[3], all ? 0 : 1, min_kinship, table.data(), table.size());
        else st = vcfc_kinship_file(ctx, argv[2], argv[3], all ? 0 : 1, min_kinship, query ? 1 : 0, q.data(), ref_len, has_range, start, end);
        vcfc_ctx_destroy(ctx);
        if (st == VCFC_E_FORMAT) {
            fprintf(stderr, "terminate called after throwing an instance of 'VcfValidationError'\n"
                            "  what():  %s\n", vcfc_strerror(st));
            return 134;
        }
        if (st != VCFC_OK) {
            fprintf(stderr, "Error in kinship of file: %s\n", vcfc_strerror(st));
            return 1;
        }
        return 0;
    }
    std::printf("Unknown action name: %s\n", action.c_str());
    return 0;
}
