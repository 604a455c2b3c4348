// kc_cli.cpp -- `kaarme` drop-in command line on top of libkc.so.
//
// Same interface as the reference's main.cpp:127-156 (CLI11 options, exactly one
// of -s/-u, -u needs -b, -f needs -b), the same input format detection
// (main.cpp:19-68), the same chunking (kc_plan_chunks == io_worker +
// read_chunk_from_file) and the same output text ("<CANONICAL_KMER> <count>\n" for
// T(c) >= a, default file "<input stem>.kaarme_counts", main.cpp:189-191).
// Exit codes of option errors follow CLI11's ExitCodes (CLI11.hpp).
//
// Deliberate differences (documented in DESIGN.md): -t defaults to 3 (the reference
// crashes without it); gzip input is decompressed completely (the reference
// truncates it); the work runs on one MI355X.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/kc_api.h"
#include "kc_unitig_host.h"
#include "kc_path_host.h"

namespace {

enum CliExit { kConversion = 104, kValidation = 105, kRequired = 106, kRequires = 107, kExcludes = 108, kExtras = 109 };

// the six options --clean-*, --pop-* and --cut-* all have: --X-max-mean, --X-rounds, --X-min, --X-max,
// --X-out, --X-stats (take_filter_opt, check_filter_opts)
struct FilterOpts {
    unsigned long long max_mean = 0, rounds = 1, min = 0, max = 0;
    bool dep_set = false, min_set = false;  // an option that needs the family's switch was given; --X-min was
    std::string out, stats;
};

struct Args {
    std::string input, output;
    long long k = 0;
    int mode = 2;
    unsigned long long min_abundance = 2;
    int threads = 3;
    bool use_bf = false;
    double fpr = 0.01;
    bool fpr_set = false;
    bool have_s = false, have_u = false;
    unsigned long long slots = 0, unique = 0;
    int device = 0;
    std::string gunzip_to;  // test hook: write the decompressed input there and exit (no GPU)
    // extensions, not in --help: --host-chunks stages host chunks instead of one
    // device image; --no-warmup skips the untimed warm-up pass; --readers N upload threads; --phases
    // prints the counting pass's phase times on stderr; --digest-only prints the output's digest
    // (kc_output_digest) instead of writing it; --table-sizing auto|s|estimate: the device table from
    // -s or from the input's distinct estimate (auto: the estimate when the -s table passes 16 GiB)
    bool host_chunks = false, no_warmup = false, phases = false, digest_only = false;
    int table_sizing = 0;  // --table-sizing auto (0) | s (1) | estimate (2)
    unsigned readers = 1;
    // extensions that query the counted table (kc_histogram / kc_lookup): --histo FILE writes the
    // abundance spectrum, --query FILE --query-out FILE answers one k-mer per line
    std::string histo, query, query_out;
    // --coverage FILE --coverage-out FILE [--coverage-min N]: per-record statistics of the k-mer
    // counts of another file's sequences (kc_seq_stats); N (a k-mer is solid from this count on)
    // defaults to the -a value
    std::string coverage, coverage_out;
    // --correct FILE --correct-out FILE [--correct-min N]: the file's sequences with their isolated
    // base errors corrected from the table (kc_correct), written back in the file's format
    std::string correct, correct_out;
    unsigned long long correct_min = 0;
    bool correct_min_set = false;
    unsigned long long coverage_min = 0;
    bool coverage_min_set = false;
    // --op NAME --with FILE2 [--a-min/--a-max/--b-min/--b-max N]: FILE2 is counted like INPUT into a
    // second table and the output is the result of the table operation (kc_table_op) on the two
    std::string op_name, with;
    int op = -1;
    unsigned long long a_min = 0, a_max = 0, b_min = 0, b_max = 0;
    bool range_set = false;
    // --graph FILE [--graph-min N] [--graph-max N] [--graph-stats FILE]: the de Bruijn graph of the
    // counted k-mers (kc_graph): a line per node with its edges and unitig links, and the graph's
    // statistics; N (a k-mer is a node when its count is in the range) defaults to the -a value and
    // to no upper bound
    std::string graph, graph_stats;
    unsigned long long graph_min = 0, graph_max = 0;
    bool graph_min_set = false, graph_max_set = false;
    // --unitigs FILE [--unitigs-min N] [--unitigs-max N]: the unitigs of that graph (kc_unitigs) as
    // FASTA, a record per unitig; the range as for --graph
    std::string unitigs;
    unsigned long long unitigs_min = 0, unitigs_max = 0;
    bool unitigs_min_set = false, unitigs_max_set = false;
    // --gfa FILE [--gfa-min N] [--gfa-max N]: the compacted graph (kc_unitig_graph) as GFA 1.0, the
    // unitigs as segments and the edges between them as links; the range as for --graph
    std::string gfa;
    // --paths FILE --paths-out FILE [--paths-stats FILE]: the records of FILE (read as --coverage's)
    // threaded through that compacted graph (kc_read_paths, the one call that then also feeds --gfa's
    // writer), as GAF: one line per chain, the segment names those of the GFA beside it
    std::string paths, paths_out, paths_stats;
    unsigned long long gfa_min = 0, gfa_max = 0;
    bool gfa_min_set = false, gfa_max_set = false;
    // --clean-tips N / --clean-isolated N [--clean-max-mean M] [--clean-rounds R] [--clean-min N]
    // [--clean-max N] [--clean-out FILE] [--clean-stats FILE]: graph cleaning (kc_clean) of the counted
    // table into a new one, R rounds at the most, which --graph, --unitigs and --gfa then read (their
    // own ranges applied to it); every other output still reads the counted table.  The range as for
    // --graph.
    unsigned long long clean_tips = 0, clean_iso = 0;
    bool clean_tips_set = false, clean_iso_set = false;
    FilterOpts clean;
    bool cleaning() const { return clean_tips_set || clean_iso_set; }
    // --pop-bubbles N [--pop-max-diff D] [--pop-max-mean M] [--pop-rounds R] [--pop-min N] [--pop-max N]
    // [--pop-out FILE] [--pop-stats FILE]: bubble popping (kc_pop_bubbles) of the counted table -- of
    // the cleaned one when --clean-* are given too -- into a new one, R rounds at the most, which
    // --graph, --unitigs and --gfa then read.  The range as for --clean-min / --clean-max.
    unsigned long long pop_nodes = 0, pop_max_diff = 0;
    bool pop_set = false;
    FilterOpts pop;
    // --cut-weak N [--cut-ratio P] [--cut-max-mean M] [--cut-rounds R] [--cut-min N] [--cut-max N]
    // [--cut-out FILE] [--cut-stats FILE]: weak-link removal (kc_cut_weak) of the counted table -- of
    // the one the --clean-* and --pop-* rounds left when those are given too -- into a new one, R
    // rounds at the most, which --graph, --unitigs and --gfa then read.  The range as for --clean-min /
    // --clean-max.
    unsigned long long cut_nodes = 0, cut_ratio = 200;
    bool cut_set = false;
    FilterOpts cut;
};

const char* const kOpNames[] = {"intersect-min", "intersect-sum", "intersect-left", "subtract",
                                "counts-subtract", "union-sum", "union-max"};  // KC_OP_* order

void usage(const char* prog) {
    std::cout << "Space-efficient k-mer counter\n"
                 "Usage: " << prog << " [OPTIONS] INPUT KLEN\n\n"
                 "Positionals:\n"
                 "  INPUT TEXT:FILE REQUIRED    Input file (automatic format detection)\n"
                 "  KLEN INT REQUIRED           k-mer length\n\n"
                 "Options:\n"
                 "  -h,--help                   Print this help message and exit\n"
                 "  -m,--hash-table-type INT    Hash table type: 0 for plain and 2 for kaarme (def. 2)\n"
                 "  -a,--min-k-abu UINT         Minimum abundance threshold for the output k-mers (def. 2)\n"
                 "  -t,--threads UINT           Number of working threads (def. 3)\n"
                 "  -o,--output-file TEXT       Output file where the k-mer counts will be stored\n"
                 "  -b,--use-bfilter            Use bloom filters to discard unique k-mers\n"
                 "  -f,--bfilter-fpr FLOAT      Bloom filter false positive rate (def. 0.01)\n"
                 "  --device INT                HIP device ordinal (def. 0)\n"
                 "  --strict-capacity           fail like the reference once the distinct k-mers pass its table\n"
                 "                              size next_prime3mod4(-s) (the device table keeps 25 % headroom)\n"
                 "  --histo FILE                write the abundance spectrum \"<count> <k-mers>\" (not filtered by -a)\n"
                 "  --query FILE                k-mers to look up, one per line (either strand, any case)\n"
                 "  --query-out FILE            their counts \"<k-mer> <count>\" (0 = absent); needed with --query\n"
                 "  --coverage FILE             sequences (FASTA, FASTQ or one per line) whose k-mers to look up\n"
                 "  --coverage-out FILE         per record, tab-separated: name length windows present solid min\n"
                 "                              median max sum (of its k-mers' counts); needed with --coverage\n"
                 "  --coverage-min UINT         a k-mer is solid from this count on (def. the -a value)\n"
                 "  --correct FILE              sequences (FASTA, FASTQ or one per line) whose isolated base errors\n"
                 "                              to correct: a base all of whose k-mers are weak and that exactly\n"
                 "                              one other base makes solid\n"
                 "  --correct-out FILE          the corrected records, in the format of FILE; needed with --correct\n"
                 "  --correct-min UINT          a k-mer is solid from this count on (def. the -a value)\n"
                 "  --op NAME                   output a table operation on INPUT (a) and the --with file (b): intersect-min,\n"
                 "                              intersect-sum, intersect-left, subtract, counts-subtract, union-sum, union-max\n"
                 "  --with FILE                 the second input, counted with the same options; needed with --op\n"
                 "  --a-min,--a-max,--b-min,--b-max UINT\n"
                 "                              a k-mer takes part when its count is in its file's range (def. 1 and up)\n"
                 "  --graph FILE                write the de Bruijn graph of the counted k-mers, a line per node:\n"
                 "                              \"<k-mer> <count> <R> <L> <links>\" -- R, L: the bases that follow and\n"
                 "                              precede it (A..T: A and T do), links: its unitig links (--, -R, L-, LR)\n"
                 "  --graph-min,--graph-max UINT\n"
                 "                              a k-mer is a node when its count is in this range (def. the -a value and\n"
                 "                              up); needs --graph\n"
                 "  --graph-stats FILE          write the graph's statistics as \"<name> <value>\" lines\n"
                 "  --unitigs FILE              write the unitigs of that graph as FASTA, a record per unitig:\n"
                 "                              \">i LN:i:<bases> KC:i:<sum of counts> km:f:<mean count>\", then\n"
                 "                              \" circular\" for a circle, and the bases on one line\n"
                 "  --unitigs-min,--unitigs-max UINT\n"
                 "                              a k-mer is a node when its count is in this range (def. the -a value and\n"
                 "                              up); needs --unitigs\n"
                 "  --gfa FILE                  write the compacted de Bruijn graph as GFA 1.0: a segment per unitig\n"
                 "                              \"S <i> <bases> LN:i:<bases> KC:i:<sum of counts>\", a link per edge\n"
                 "                              between unitigs \"L <i> <+|-> <j> <+|-> <k-1>M\", and the two links\n"
                 "                              \"L i + i +\", \"L i - i -\" that close a circular unitig\n"
                 "  --gfa-min,--gfa-max UINT    a k-mer is a node when its count is in this range (def. the -a value and\n"
                 "                              up); needs --gfa\n"
                 "  --paths FILE                sequences (FASTA, FASTQ or one per line) to thread through that graph;\n"
                 "                              needs --gfa (the segment names are that file's) and --paths-out\n"
                 "  --paths-out FILE            GAF, a line per chain of consecutive located k-mers: name qlen qstart\n"
                 "                              qend + path plen pstart pend matches alnlen 255 cg:Z:<alnlen>=\n"
                 "  --paths-stats FILE          the totals, one per line: seqs windows located runs chains threaded;\n"
                 "                              needs --paths\n"
                 "  --clean-tips UINT           clean the graph first: remove the dead-end branches (tips) of at most this\n"
                 "                              many k-mers (k - 1 is customary; 0 keeps them); --graph, --unitigs and\n"
                 "                              --gfa then read the cleaned table, every other output the counted one\n"
                 "  --clean-isolated UINT       ... and the unitigs connected to nothing of at most this many k-mers\n"
                 "  --clean-max-mean UINT       never remove a unitig whose mean count is above this (def. no guard)\n"
                 "  --clean-rounds UINT         cleaning rounds, each on the result of the one before; they stop early\n"
                 "                              after a round that removes nothing (def. 1)\n"
                 "  --clean-min,--clean-max UINT\n"
                 "                              a k-mer is a node when its count is in this range (def. the -a value and up)\n"
                 "  --clean-out FILE            write every k-mer of the cleaned table, as -o writes the counted one's\n"
                 "  --clean-stats FILE          a line of \"<name> <value>\" pairs per round\n"
                 "  --pop-bubbles UINT          pop the graph's bubbles (after the --clean-* rounds, on the table those\n"
                 "                              left): of the unitigs of at most this many k-mers (k is customary) that\n"
                 "                              run between the same two unitig ends, all but the one with the highest\n"
                 "                              mean count go; --graph, --unitigs and --gfa then read the result\n"
                 "  --pop-max-diff UINT         ... when their lengths differ by at most this many k-mers (def. 0)\n"
                 "  --pop-max-mean UINT         never pop a unitig whose mean count is above this (def. no guard)\n"
                 "  --pop-rounds UINT           popping rounds, each on the result of the one before; they stop early\n"
                 "                              after a round that pops nothing (def. 1)\n"
                 "  --pop-min,--pop-max UINT    a k-mer is a node when its count is in this range (def. the -a value and up)\n"
                 "  --pop-out FILE              write every k-mer of the popped table, as -o writes the counted one's\n"
                 "  --pop-stats FILE            a line of \"<name> <value>\" pairs per round\n"
                 "  --cut-weak UINT             cut the graph's weak links (after the --clean-* and --pop-* rounds, on the\n"
                 "                              table those left): a unitig of at most this many k-mers (k to 2 k is\n"
                 "                              customary) that is connected at both ends goes when its mean count is\n"
                 "                              low beside its neighbours'; --graph, --unitigs and --gfa then read the result\n"
                 "  --cut-ratio UINT            ... below this many thousandths of the mean count of the unitigs around\n"
                 "                              it (def. 200; at most 1000; from about 500 both arms of a bubble go;\n"
                 "                              0: no such test, --cut-max-mean alone decides)\n"
                 "  --cut-max-mean UINT         never cut a unitig whose mean count is above this (def. no guard)\n"
                 "  --cut-rounds UINT           cutting rounds, each on the result of the one before; they stop early\n"
                 "                              after a round that cuts nothing (def. 1)\n"
                 "  --cut-min,--cut-max UINT    a k-mer is a node when its count is in this range (def. the -a value and up)\n"
                 "  --cut-out FILE              write every k-mer of the cut table, as -o writes the counted one's\n"
                 "  --cut-stats FILE            a line of \"<name> <value>\" pairs per round\n\n"
                 "Mandatory params:\n"
                 "  -s,--hash-tab-size UINT     Hash table size\n"
                 "  -u,--unq-kmers UINT         Estimated number of unique k-mers\n";
}

int cli_error(int code, const std::string& msg) {
    std::cerr << msg << "\nRun with --help for more information.\n";
    return code;
}

bool parse_uint(const std::string& s, unsigned long long* v) {
    if (s.empty() || s[0] == '-' || s[0] == '+') return false;
    char* end = nullptr;
    errno = 0;
    *v = std::strtoull(s.c_str(), &end, 10);
    return errno == 0 && end && *end == 0;
}
bool parse_int(const std::string& s, long long* v) {
    if (s.empty()) return false;
    char* end = nullptr;
    errno = 0;
    *v = std::strtoll(s.c_str(), &end, 10);
    return errno == 0 && end && *end == 0;
}
bool parse_double(const std::string& s, double* v) {
    if (s.empty()) return false;
    char* end = nullptr;
    *v = std::strtod(s.c_str(), &end);
    return end && *end == 0;
}

// o = v as one of FilterOpts' six under `prefix` ("--clean-", "--pop-", "--cut-"): 1 taken, 0 not one of them,
// -1 one of them whose value is no 32-bit number
int take_filter_opt(FilterOpts* f, const std::string& prefix, const std::string& o, const std::string& v) {
    const std::string name = o.compare(0, prefix.size(), prefix) == 0 ? o.substr(prefix.size()) : "";
    unsigned long long* num = name == "max-mean" ? &f->max_mean : name == "rounds" ? &f->rounds
                              : name == "min"    ? &f->min : name == "max" ? &f->max : nullptr;
    std::string* text = name == "out" ? &f->out : name == "stats" ? &f->stats : nullptr;
    if (!num && !text) return 0;
    if (num && (!parse_uint(v, num) || *num > 0xFFFFFFFFull)) return -1;
    if (text) *text = v;
    f->dep_set = true;
    f->min_set |= name == "min";
    return 1;
}

// What every family checks once all options are read (on: the family's switch was given); the
// range's default as for --graph-min.  -1: fine, else the exit code.
int check_filter_opts(FilterOpts* f, bool on, const std::string& prefix, const Args& a, const char* requires_text,
                      const char* excludes_text) {
    if (f->dep_set && !on) return cli_error(kRequires, requires_text);
    if (!f->min_set) f->min = std::min<unsigned long long>(a.min_abundance, 0xFFFFFFFFull);
    if (f->max && f->min > f->max) return cli_error(kValidation, prefix + "min: a minimum above its maximum");
    if (f->rounds < 1) return cli_error(kValidation, prefix + "rounds: Value 0 not in range 1 to inf");
    if (on && !a.op_name.empty()) return cli_error(kExcludes, excludes_text);
    return -1;
}

// BGZF input (blocked gzip, bgzip / htslib: every member carries its compressed size in a
// 'BC' extra subfield and is at most 64 KiB uncompressed): the members are inflated by up to
// `nt` threads straight into their slots of one buffer (each member's ISIZE gives its slot).
// Returns false when the file is not BGZF (the caller reads it as one stream); *bad is set
// when a member does not inflate to its ISIZE (corrupt input).
static bool gunzip_bgzf(const uint8_t* z, uint64_t n, int nt, std::vector<uint8_t>* out, bool* bad) {
    std::vector<uint64_t> off, len, dst;
    std::vector<uint32_t> usz;
    uint64_t p = 0, total = 0;
    while (p < n) {
        if (n - p < 28 || z[p] != 0x1f || z[p + 1] != 0x8b || z[p + 2] != 8 || !(z[p + 3] & 4)) return false;
        const uint32_t xlen = z[p + 10] | (uint32_t)z[p + 11] << 8;
        if (12 + (uint64_t)xlen > n - p) return false;
        uint64_t bsize = 0;
        for (uint32_t q = 0; q + 4 <= xlen;) {
            const uint8_t* f = z + p + 12 + q;
            const uint32_t sl = f[2] | (uint32_t)f[3] << 8;
            if (f[0] == 'B' && f[1] == 'C' && sl == 2 && q + 6 <= xlen) {
                bsize = (f[4] | (uint32_t)f[5] << 8) + 1ULL;
                break;
            }
            q += 4 + sl;
        }
        if (bsize < 20 + (uint64_t)xlen || bsize > n - p) return false;
        const uint8_t* t = z + p + bsize - 4;
        const uint32_t isz = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        if (isz > 65536) {  // a BGZF member holds at most 64 KiB: a forged or corrupt ISIZE
            *bad = true;
            return true;
        }
        off.push_back(p);
        len.push_back(bsize);
        usz.push_back(isz);
        dst.push_back(total);
        total += isz;
        p += bsize;
    }
    if (off.size() < 2) return false;  // one member: nothing to split
    try {
        out->resize(total);
    } catch (const std::bad_alloc&) {
        *bad = true;
        return true;
    }
    std::atomic<uint64_t> next{0};
    std::atomic<bool> fail{false};
    auto work = [&]() {
        uint8_t dummy = 0;
        for (uint64_t i; (i = next.fetch_add(1)) < off.size() && !fail.load();) {
            z_stream st{};
            if (inflateInit2(&st, 16 + MAX_WBITS) != Z_OK) { fail = true; break; }
            st.next_in = const_cast<Bytef*>(z + off[i]);
            st.avail_in = (uInt)len[i];
            st.next_out = usz[i] ? out->data() + dst[i] : &dummy;
            st.avail_out = usz[i] ? usz[i] : 1;
            const int r = inflate(&st, Z_FINISH);
            if (r != Z_STREAM_END || st.total_out != usz[i] || st.avail_in != 0) fail = true;
            inflateEnd(&st);
        }
    };
    const int T = std::max(1, std::min<int>(nt, (int)std::min<uint64_t>(off.size(), 64)));
    std::vector<std::thread> th;
    for (int i = 1; i < T; i++) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
    *bad = fail.load();
    return true;
}

// returns -1 on success, else exit code
int parse(int argc, char** argv, Args* a) {
    std::vector<std::string> pos;
    for (int i = 1; i < argc; i++) {
        std::string o = argv[i];
        std::string val;
        bool has_inline = false;
        if (o.rfind("--", 0) == 0 && o.find('=') != std::string::npos) {
            val = o.substr(o.find('=') + 1);
            o = o.substr(0, o.find('='));
            has_inline = true;
        }
        auto next = [&](std::string* out) -> bool {
            if (has_inline) { *out = val; return true; }
            if (i + 1 >= argc) return false;
            *out = argv[++i];
            return true;
        };
        if (o == "-h" || o == "--help") { usage(argv[0]); return 0; }
        if (o == "-b" || o == "--use-bfilter") { a->use_bf = true; continue; }
        if (o == "--strict-capacity") { setenv("KC_STRICT_CAPACITY", "1", 1); continue; }  // kc_api.h
        if (o == "--host-chunks") { a->host_chunks = true; continue; }
        if (o == "--no-warmup") { a->no_warmup = true; continue; }
        if (o == "--phases") { a->phases = true; continue; }
        if (o == "--digest-only") { a->digest_only = true; continue; }
        if (o.size() > 1 && o[0] == '-' && !(o.size() > 1 && std::isdigit((unsigned char)o[1]))) {
            std::string v;
            if (!next(&v)) return cli_error(kRequired, o + " requires an argument");
            unsigned long long u;
            long long si;
            double d;
            if (o == "-m" || o == "--hash-table-type") {
                if (!parse_int(v, &si)) return cli_error(kConversion, "Could not convert: " + o + " = " + v);
                if (si < 0 || si > 2) return cli_error(kValidation, o + ": Value " + v + " not in range 0 to 2");
                a->mode = (int)si;
            } else if (o == "-a" || o == "--min-k-abu") {
                if (!parse_uint(v, &u)) return cli_error(kConversion, "Could not convert: " + o + " = " + v);
                a->min_abundance = u;
            } else if (o == "-t" || o == "--threads") {
                if (!parse_int(v, &si)) return cli_error(kConversion, "Could not convert: " + o + " = " + v);
                if (si < 3 || si > 64) return cli_error(kValidation, o + ": Value " + v + " not in range 3 to 64");
                a->threads = (int)si;
            } else if (o == "-o" || o == "--output-file") {
                a->output = v;
            } else if (o == "-f" || o == "--bfilter-fpr") {
                if (!parse_double(v, &d)) return cli_error(kConversion, "Could not convert: " + o + " = " + v);
                if (!(d >= 0.001 && d <= 0.999))
                    return cli_error(kValidation, o + ": Value " + v + " not in range 0.001 to 0.999");
                a->fpr = d;
                a->fpr_set = true;
            } else if (o == "-s" || o == "--hash-tab-size") {
                if (!parse_uint(v, &u)) return cli_error(kConversion, "Could not convert: " + o + " = " + v);
                a->slots = u;
                a->have_s = true;
            } else if (o == "-u" || o == "--unq-kmers") {
                if (!parse_uint(v, &u)) return cli_error(kConversion, "Could not convert: " + o + " = " + v);
                a->unique = u;
                a->have_u = true;
            } else if (o == "--gunzip-to") {
                a->gunzip_to = v;
            } else if (o == "--device") {
                if (!parse_int(v, &si) || si < 0) return cli_error(kConversion, "Could not convert: " + o + " = " + v);
                a->device = (int)si;
            } else if (o == "--table-sizing") {
                if (v == "auto") a->table_sizing = 0;
                else if (v == "s") a->table_sizing = 1;
                else if (v == "estimate") a->table_sizing = 2;
                else return cli_error(kValidation, o + ": Value " + v + " not in {auto, s, estimate}");
            } else if (o == "--histo") {
                a->histo = v;
            } else if (o == "--query") {
                a->query = v;
            } else if (o == "--query-out") {
                a->query_out = v;
            } else if (o == "--coverage") {
                a->coverage = v;
            } else if (o == "--coverage-out") {
                a->coverage_out = v;
            } else if (o == "--coverage-min") {
                if (!parse_uint(v, &u) || u > 0xFFFFFFFFull)
                    return cli_error(kConversion, "Could not convert: " + o + " = " + v);
                a->coverage_min = u;
                a->coverage_min_set = true;
            } else if (o == "--correct") {
                a->correct = v;
            } else if (o == "--correct-out") {
                a->correct_out = v;
            } else if (o == "--correct-min") {
                if (!parse_uint(v, &u) || u > 0xFFFFFFFFull)
                    return cli_error(kConversion, "Could not convert: " + o + " = " + v);
                a->correct_min = u;
                a->correct_min_set = true;
            } else if (o == "--graph") {
                a->graph = v;
            } else if (o == "--graph-stats") {
                a->graph_stats = v;
            } else if (o == "--graph-min" || o == "--graph-max") {
                if (!parse_uint(v, &u) || u > 0xFFFFFFFFull)
                    return cli_error(kConversion, "Could not convert: " + o + " = " + v);
                (o == "--graph-min" ? a->graph_min : a->graph_max) = u;
                (o == "--graph-min" ? a->graph_min_set : a->graph_max_set) = true;
            } else if (o == "--unitigs") {
                a->unitigs = v;
            } else if (o == "--unitigs-min" || o == "--unitigs-max") {
                if (!parse_uint(v, &u) || u > 0xFFFFFFFFull)
                    return cli_error(kConversion, "Could not convert: " + o + " = " + v);
                (o == "--unitigs-min" ? a->unitigs_min : a->unitigs_max) = u;
                (o == "--unitigs-min" ? a->unitigs_min_set : a->unitigs_max_set) = true;
            } else if (o == "--gfa") {
                a->gfa = v;
            } else if (o == "--paths") {
                a->paths = v;
            } else if (o == "--paths-out") {
                a->paths_out = v;
            } else if (o == "--paths-stats") {
                a->paths_stats = v;
            } else if (o == "--gfa-min" || o == "--gfa-max") {
                if (!parse_uint(v, &u) || u > 0xFFFFFFFFull)
                    return cli_error(kConversion, "Could not convert: " + o + " = " + v);
                (o == "--gfa-min" ? a->gfa_min : a->gfa_max) = u;
                (o == "--gfa-min" ? a->gfa_min_set : a->gfa_max_set) = true;
            } else if (int t = take_filter_opt(&a->clean, "--clean-", o, v) | take_filter_opt(&a->pop, "--pop-", o, v) |
                               take_filter_opt(&a->cut, "--cut-", o, v)) {
                if (t < 0) return cli_error(kConversion, "Could not convert: " + o + " = " + v);  // (the other calls gave 0)
            } else if (o == "--clean-tips" || o == "--clean-isolated" || o == "--pop-bubbles" || o == "--pop-max-diff" ||
                       o == "--cut-weak" || o == "--cut-ratio") {
                if (!parse_uint(v, &u) || u > 0xFFFFFFFFull)
                    return cli_error(kConversion, "Could not convert: " + o + " = " + v);
                (o == "--clean-tips" ? a->clean_tips : o == "--clean-isolated" ? a->clean_iso
                 : o == "--pop-bubbles" ? a->pop_nodes : o == "--pop-max-diff" ? a->pop_max_diff
                 : o == "--cut-weak" ? a->cut_nodes : a->cut_ratio) = u;
                (o == "--clean-tips" ? a->clean_tips_set : o == "--clean-isolated" ? a->clean_iso_set
                 : o == "--pop-bubbles" ? a->pop_set : o == "--pop-max-diff" ? a->pop.dep_set
                 : o == "--cut-weak" ? a->cut_set : a->cut.dep_set) = true;
            } else if (o == "--op") {
                a->op_name = v;
                for (int q = 0; q < 7; q++)
                    if (v == kOpNames[q]) a->op = q;
                if (a->op < 0)
                    return cli_error(kValidation, o + ": Value " + v + " not in {intersect-min, intersect-sum, "
                                                  "intersect-left, subtract, counts-subtract, union-sum, union-max}");
            } else if (o == "--with") {
                a->with = v;
            } else if (o == "--a-min" || o == "--a-max" || o == "--b-min" || o == "--b-max") {
                if (!parse_uint(v, &u) || u > 0xFFFFFFFFull)
                    return cli_error(kConversion, "Could not convert: " + o + " = " + v);
                (o == "--a-min" ? a->a_min : o == "--a-max" ? a->a_max : o == "--b-min" ? a->b_min : a->b_max) = u;
                a->range_set = true;
            } else if (o == "--readers") {
                if (!parse_int(v, &si) || si < 1 || si > 16) return cli_error(kConversion, "Could not convert: " + o + " = " + v);
                a->readers = (unsigned)si;
            } else {
                return cli_error(kExtras, "The following argument was not expected: " + o);
            }
            continue;
        }
        pos.push_back(o);
    }
    if (pos.size() > 2) return cli_error(kExtras, "The following arguments were not expected: " + pos[2]);
    if (pos.size() < 1) return cli_error(kRequired, "INPUT is required");
    if (pos.size() < 2) return cli_error(kRequired, "KLEN is required");
    a->input = pos[0];
    struct stat st;
    if (stat(a->input.c_str(), &st) != 0 || S_ISDIR(st.st_mode))
        return cli_error(kValidation, "INPUT: File does not exist: " + a->input);
    if (!parse_int(pos[1], &a->k)) return cli_error(kConversion, "Could not convert: KLEN = " + pos[1]);
    if (a->k <= 0) return cli_error(kValidation, "KLEN: Value " + pos[1] + " not in range 0 to inf");
    if (a->have_s == a->have_u)
        return cli_error(kRequired, "[Option Group: dummy group2] Exactly 1 option from [-s,--hash-tab-size,-u,--unq-kmers] is required");
    if (a->use_bf && !a->have_u) return cli_error(kRequires, "--use-bfilter requires --unq-kmers");
    if (a->have_u && !a->use_bf) return cli_error(kRequires, "--unq-kmers requires --use-bfilter");
    if (a->fpr_set && !a->use_bf) return cli_error(kRequires, "--bfilter-fpr requires --use-bfilter");
    if (!a->query.empty() && a->query_out.empty()) return cli_error(kRequires, "--query requires --query-out");
    if (a->query.empty() && !a->query_out.empty()) return cli_error(kRequires, "--query-out requires --query");
    if (!a->coverage.empty() && a->coverage_out.empty())
        return cli_error(kRequires, "--coverage requires --coverage-out");
    if (a->coverage.empty() && !a->coverage_out.empty())
        return cli_error(kRequires, "--coverage-out requires --coverage");
    if (a->coverage_min_set && a->coverage.empty()) return cli_error(kRequires, "--coverage-min requires --coverage");
    if (!a->coverage_min_set) a->coverage_min = std::min<unsigned long long>(a->min_abundance, 0xFFFFFFFFull);
    if (!a->correct.empty() && a->correct_out.empty()) return cli_error(kRequires, "--correct requires --correct-out");
    if (a->correct.empty() && !a->correct_out.empty()) return cli_error(kRequires, "--correct-out requires --correct");
    if (a->correct_min_set && a->correct.empty()) return cli_error(kRequires, "--correct-min requires --correct");
    if (!a->correct_min_set) a->correct_min = std::min<unsigned long long>(a->min_abundance, 0xFFFFFFFFull);
    if ((a->graph_min_set || a->graph_max_set) && a->graph.empty())
        return cli_error(kRequires, "--graph-min/--graph-max require --graph");
    if (!a->graph_min_set) a->graph_min = std::min<unsigned long long>(a->min_abundance, 0xFFFFFFFFull);
    if (a->graph_max && a->graph_min > a->graph_max)
        return cli_error(kValidation, "--graph-min: a minimum above its maximum");
    if ((a->unitigs_min_set || a->unitigs_max_set) && a->unitigs.empty())
        return cli_error(kRequires, "--unitigs-min/--unitigs-max require --unitigs");
    if (!a->unitigs_min_set) a->unitigs_min = std::min<unsigned long long>(a->min_abundance, 0xFFFFFFFFull);
    if (a->unitigs_max && a->unitigs_min > a->unitigs_max)
        return cli_error(kValidation, "--unitigs-min: a minimum above its maximum");
    if ((a->gfa_min_set || a->gfa_max_set) && a->gfa.empty())
        return cli_error(kRequires, "--gfa-min/--gfa-max require --gfa");
    if (!a->paths.empty() && a->gfa.empty()) return cli_error(kRequires, "--paths requires --gfa");
    if (!a->paths.empty() && a->paths_out.empty()) return cli_error(kRequires, "--paths requires --paths-out");
    if (a->paths.empty() && !a->paths_out.empty()) return cli_error(kRequires, "--paths-out requires --paths");
    if (a->paths.empty() && !a->paths_stats.empty()) return cli_error(kRequires, "--paths-stats requires --paths");
    if (!a->gfa_min_set) a->gfa_min = std::min<unsigned long long>(a->min_abundance, 0xFFFFFFFFull);
    if (a->gfa_max && a->gfa_min > a->gfa_max) return cli_error(kValidation, "--gfa-min: a minimum above its maximum");
    int bad = check_filter_opts(&a->clean, a->cleaning(), "--clean-", *a,
                                "--clean-max-mean/--clean-rounds/--clean-min/--clean-max/--clean-out/--clean-stats "
                                "require --clean-tips or --clean-isolated", "--clean-tips/--clean-isolated exclude --op");
    if (bad >= 0) return bad;
    bad = check_filter_opts(&a->pop, a->pop_set, "--pop-", *a,
                            "--pop-max-diff/--pop-max-mean/--pop-rounds/--pop-min/--pop-max/--pop-out/--pop-stats "
                            "require --pop-bubbles", "--pop-bubbles excludes --op");
    if (bad >= 0) return bad;
    bad = check_filter_opts(&a->cut, a->cut_set, "--cut-", *a,
                            "--cut-ratio/--cut-max-mean/--cut-rounds/--cut-min/--cut-max/--cut-out/--cut-stats "
                            "require --cut-weak", "--cut-weak excludes --op");
    if (bad >= 0) return bad;
    if (a->cut_ratio > 1000)
        return cli_error(kValidation, "--cut-ratio: Value " + std::to_string(a->cut_ratio) + " not in range 0 to 1000");
    if (!a->op_name.empty() && a->with.empty()) return cli_error(kRequires, "--op requires --with");
    if (a->op_name.empty() && !a->with.empty()) return cli_error(kRequires, "--with requires --op");
    if (a->range_set && a->op_name.empty()) return cli_error(kRequires, "--a-min/--a-max/--b-min/--b-max require --op");
    if ((a->a_max && a->a_min > a->a_max) || (a->b_max && a->b_min > a->b_max))
        return cli_error(kValidation, "--a-min/--b-min: a minimum above its maximum");
    if (!a->with.empty() && (stat(a->with.c_str(), &st) != 0 || S_ISDIR(st.st_mode)))
        return cli_error(kValidation, "--with: File does not exist: " + a->with);
    return -1;
}

std::string ext_of(const std::string& p) {  // std::filesystem::path::extension()
    size_t slash = p.find_last_of('/');
    std::string fn = slash == std::string::npos ? p : p.substr(slash + 1);
    size_t dot = fn.find_last_of('.');
    if (dot == std::string::npos || dot == 0 || fn == "..") return "";
    return fn.substr(dot);
}
std::string stem_of(const std::string& p) {
    size_t slash = p.find_last_of('/');
    std::string fn = slash == std::string::npos ? p : p.substr(slash + 1);
    size_t dot = fn.find_last_of('.');
    if (dot == std::string::npos || dot == 0) return fn;
    return fn.substr(0, dot);
}
std::string filename_of(const std::string& p) {
    size_t slash = p.find_last_of('/');
    return slash == std::string::npos ? p : p.substr(slash + 1);
}

// The input image in HBM: slices of the file (pread, fd >= 0) or of a host buffer
// (decompressed gzip) are copied by `readers` workers, each through two pinned slices and
// its own stream, so reading, H2D and the next read overlap.  prepare() allocates the image,
// the pinned slices, streams and events before the timed passes (as the reference allocates its
// table before its timer, parallel_parser.hpp:1230-1299): page-locking the slices was most of
// the upload's time.  run() then only reads and copies.  prepare() returns
// false (the caller stages host chunks instead) when the image does not fit comfortably in HBM.
struct Upload {
    uint8_t* d = nullptr;
    uint64_t size = 0, slice = 0, nslices = 0;
    struct Reader {
        hipStream_t st = nullptr;
        uint8_t* buf[2] = {nullptr, nullptr};
        hipEvent_t done[2] = {nullptr, nullptr};
    };
    std::vector<Reader> rd;
    // one reader: an event per slice and the slices issued so far (in file order), so that the
    // counting pass of a prefix can start while the rest uploads (wait_prefix)
    std::vector<hipEvent_t> sev;
    uint64_t issued = 0;
    bool failed = false;
    std::mutex mu;
    std::condition_variable cv;

    bool prepare(uint64_t sz, int device, unsigned readers) {
        size = sz;
        if (size == 0 || hipSetDevice(device) != hipSuccess) return false;
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess || size > fr / 4) return false;  // room for the passes
        if (hipMalloc(&d, size) != hipSuccess) {
            d = nullptr;
            return false;
        }
        slice = 8ull << 20;
        nslices = (size + slice - 1) / slice;
        readers = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(readers, nslices));
        // a slice per buffer no larger than the image: small inputs pin little
        const uint64_t bsz = std::min(slice, size);
        rd.resize(readers);
        if (readers == 1) {
            sev.assign(nslices, nullptr);
            for (auto& e : sev)
                if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail();
        }
        for (auto& r : rd) {
            if (hipStreamCreateWithFlags(&r.st, hipStreamNonBlocking) != hipSuccess) return fail();
            for (int b = 0; b < 2; b++)
                if (hipHostMalloc(&r.buf[b], bsz, hipHostMallocDefault) != hipSuccess ||
                    hipEventCreateWithFlags(&r.done[b], hipEventDisableTiming) != hipSuccess)
                    return fail();
        }
        return true;
    }
    bool release() {
        for (auto& e : sev)
            if (e) (void)hipEventDestroy(e);
        sev.clear();
        for (auto& r : rd) {
            for (int b = 0; b < 2; b++) {
                if (r.buf[b]) (void)hipHostFree(r.buf[b]);
                if (r.done[b]) (void)hipEventDestroy(r.done[b]);
                r.buf[b] = nullptr;
                r.done[b] = nullptr;
            }
            if (r.st) (void)hipStreamDestroy(r.st);
            r.st = nullptr;
        }
        rd.clear();
        return false;
    }
    void free_image() {
        if (d) (void)hipFree(d);
        d = nullptr;
    }
    bool fail() {
        release();
        free_image();
        return false;
    }
    // waits until the first `bytes` of the image are in HBM; false if the upload failed
    bool wait_prefix(uint64_t bytes) {
        const uint64_t need = std::min(nslices, (bytes + slice - 1) / slice);
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return failed || issued >= need; });
        if (failed) return false;
        lk.unlock();
        return need == 0 || hipEventSynchronize(sev[need - 1]) == hipSuccess;
    }
    // the image's bytes into d; false on a read or copy error (d is then freed unless keep_image:
    // a caller counting a prefix meanwhile frees it)
    bool run(int fd, const uint8_t* host, bool keep_image = false) {
        std::atomic<uint64_t> next{0};
        std::atomic<bool> bad{false};
        auto worker = [&](Reader& r) {
            bool ok = true, used[2] = {false, false};
            for (int b = 0; ok && !bad;) {
                const uint64_t i = next.fetch_add(1);
                if (i >= nslices) break;
                const uint64_t off = i * slice, len = std::min(slice, size - off);
                if (used[b] && hipEventSynchronize(r.done[b]) != hipSuccess) { ok = false; break; }
                if (fd >= 0) {
                    uint64_t got = 0;
                    while (got < len) {
                        const ssize_t n = pread(fd, r.buf[b] + got, len - got, (off_t)(off + got));
                        if (n <= 0) { ok = false; break; }
                        got += (uint64_t)n;
                    }
                } else {
                    std::memcpy(r.buf[b], host + off, len);
                }
                ok = ok && hipMemcpyAsync(d + off, r.buf[b], len, hipMemcpyHostToDevice, r.st) == hipSuccess &&
                     hipEventRecord(r.done[b], r.st) == hipSuccess;
                if (ok && !sev.empty()) {
                    ok = hipEventRecord(sev[i], r.st) == hipSuccess;
                    std::lock_guard<std::mutex> lk(mu);
                    issued = i + 1;
                    cv.notify_all();
                }
                used[b] = true;
                b ^= 1;
            }
            if (hipStreamSynchronize(r.st) != hipSuccess) ok = false;
            if (!ok) bad = true;
        };
        std::vector<std::thread> pool;
        for (size_t t = 1; t < rd.size(); t++) pool.emplace_back(worker, std::ref(rd[t]));
        worker(rd[0]);
        for (auto& t : pool) t.join();
        if (bad) {
            std::lock_guard<std::mutex> lk(mu);
            failed = true;
            cv.notify_all();
        }
        if (!bad) release();  // (after a failure a waiter may still hold a slice event)
        if (bad && !keep_image) free_image();
        return !bad;
    }
};

// --query FILE: one k-mer per line (A/C/G/T in any case, either strand; CRLF tolerated, empty
// lines skipped) -> the lines as given and their keys in the kc_dump layout, W words each.  A line
// of length k with another character gets a key that is no k-mer (bit 63 of word 0), which
// kc_lookup answers with 0.  Returns -1 on success, else the exit code (a line of another
// length is a usage error).
int read_queries(const std::string& path, int k, std::vector<std::string>* lines, std::vector<uint64_t>* keys) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return cli_error(kValidation, "--query: File does not exist: " + path);
    const int W = k / 32 + 1;
    std::string line;
    unsigned long long lineno = 0;
    bool eof = false;
    while (!eof) {
        line.clear();
        int ch;
        while ((ch = std::fgetc(f)) != EOF && ch != '\n') line.push_back((char)ch);
        eof = ch == EOF;
        if (eof && line.empty()) break;
        lineno++;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        if (line.size() != (size_t)k) {
            std::fclose(f);
            return cli_error(kValidation, "--query: line " + std::to_string(lineno) + " of " + path + " has " +
                                              std::to_string(line.size()) + " characters, not k = " + std::to_string(k));
        }
        const size_t base = keys->size();
        keys->resize(base + W, 0);
        bool ok = true;
        for (int j = 0; j < k; j++) {
            uint64_t c;
            switch (line[j]) {
            case 'A': case 'a': c = 0; break;
            case 'C': case 'c': c = 1; break;
            case 'G': case 'g': c = 2; break;
            case 'T': case 't': c = 3; break;
            default: c = 0; ok = false;
            }
            const int bit = 2 * (k - 1 - j);
            (*keys)[base + W - 1 - bit / 64] |= c << (bit % 64);
        }
        if (!ok) (*keys)[base] |= 1ULL << 63;
        lines->push_back(line);
    }
    std::fclose(f);
    return -1;
}

// --coverage FILE: the records of a FASTA (multi-line records joined), FASTQ (four-line records)
// or one-sequence-per-line file, the format detected as the input's is (extension and first byte;
// not gzip).  The sequences go into one text, a newline after each -- a break byte, so no k-mer
// spans two records -- with offsets[i] the start of record i (kc_seq_stats).  A record's name is
// its header's first whitespace-delimited token without the '>' or '@'; in a plain file its
// 1-based line number.  Returns -1 on success, else the exit code.
// --correct FILE reads its records the same way (opt names the option in the messages) and writes
// them back in the file's format, so the whole header lines and a FASTQ record's '+' and quality
// lines are kept too (without their CR).
struct Coverage {
    std::string text;
    std::vector<uint64_t> offsets;
    std::vector<std::string> names;
    std::vector<uint64_t> lengths;
    int fmt = KC_FMT_PLAIN;
    std::vector<std::string> headers, plus, quals;
};
int read_coverage(const std::string& path, Coverage* cv, const std::string& opt = "--coverage") {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return cli_error(kValidation, opt + ": File does not exist: " + path);
    std::string data;
    char buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) data.append(buf, got);
    std::fclose(f);
    if (data.size() >= 2 && (unsigned char)data[0] == 0x1f && (unsigned char)data[1] == 0x8b)
        return cli_error(kValidation, opt + ": gzip input is not supported: " + path);
    const std::string ext = ext_of(path);
    const unsigned char sym = data.empty() ? 0 : (unsigned char)data[0];
    int fmt;
    bool ill;
    if (ext == ".fasta" || ext == ".fa") { fmt = KC_FMT_FASTA; ill = sym != '>'; }
    else if (ext == ".fastq" || ext == ".fq") { fmt = KC_FMT_FASTQ; ill = sym != '@'; }
    else { fmt = KC_FMT_PLAIN; ill = !(sym && std::strchr("actgACGT", sym)); }
    if (ill) return cli_error(kValidation, opt + ": Input file " + path + " is ill-formed");
    cv->fmt = fmt;
    auto name_of = [](const std::string& header) {
        size_t e = 1;
        while (e < header.size() && !std::isspace((unsigned char)header[e])) e++;
        return header.substr(1, e - 1);
    };
    auto open_record = [&](const std::string& name) {
        cv->names.push_back(name);
        cv->offsets.push_back(cv->text.size());
        cv->lengths.push_back(0);
    };
    auto add_sequence = [&](const std::string& line) {
        cv->text += line;
        cv->lengths.back() += line.size();
    };
    auto close_record = [&] { cv->text.push_back('\n'); };
    unsigned long long lineno = 0;
    int phase = 0;  // FASTQ: the line of the record (0 header, 1 sequence, 2 '+', 3 qualities)
    bool in_record = false;
    for (size_t pos = 0; pos < data.size();) {
        size_t nl = data.find('\n', pos);
        if (nl == std::string::npos) nl = data.size();
        std::string line = data.substr(pos, nl - pos);
        pos = nl + 1;
        lineno++;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (fmt == KC_FMT_FASTA) {
            if (!line.empty() && line[0] == '>') {
                if (in_record) close_record();
                open_record(name_of(line));
                cv->headers.push_back(line);
                in_record = true;
            } else if (in_record) {
                add_sequence(line);
            }
        } else if (fmt == KC_FMT_FASTQ) {
            if (phase == 0 && line.empty()) continue;
            if (phase == 0) {
                if (line[0] != '@')
                    return cli_error(kValidation, opt + ": line " + std::to_string(lineno) + " of " + path +
                                                      " is not a FASTQ header");
                open_record(name_of(line));
                cv->headers.push_back(line);
            } else if (phase == 1) {
                add_sequence(line);
                close_record();
            } else if (phase == 2) {
                cv->plus.push_back(line);
            } else {
                cv->quals.push_back(line);
            }
            phase = (phase + 1) & 3;
        } else if (!line.empty()) {
            open_record(std::to_string(lineno));
            add_sequence(line);
            close_record();
        }
    }
    if (fmt == KC_FMT_FASTA && in_record) close_record();
    if (fmt == KC_FMT_FASTQ && phase == 1) close_record();  // (a header with nothing after it)
    cv->offsets.push_back(cv->text.size());
    if (fmt == KC_FMT_FASTQ) {  // (a last record cut short)
        cv->plus.resize(cv->names.size(), "+");
        cv->quals.resize(cv->names.size());
    }
    return -1;
}

// --with FILE2: the second operand of --op, counted like INPUT -- the same k, -m, -s or -b -u -f, the
// format detected the same way, gzip inflated -- into a context of its own, through staged host
// chunks.  Returns nullptr after it has printed what failed.
kc_ctx* count_with(const Args& a, kc_config cfg) {
    unsigned char magic[2] = {0, 0};
    if (FILE* f = std::fopen(a.with.c_str(), "rb")) {
        size_t r = std::fread(magic, 1, 2, f);
        (void)r;
        std::fclose(f);
    }
    const bool gz = magic[0] == 0x1f && magic[1] == 0x8b;
    gzFile g = gzopen(a.with.c_str(), "rb");  // (an uncompressed file is read as it is)
    if (!g) { std::cerr << "cannot open " << a.with << "\n"; return nullptr; }
    gzbuffer(g, 1 << 20);
    std::vector<uint8_t> img, tmp(1 << 22);
    int n;
    while ((n = gzread(g, tmp.data(), (unsigned)tmp.size())) > 0) img.insert(img.end(), tmp.begin(), tmp.begin() + n);
    int zerr = Z_OK;
    const char* msg = gzerror(g, &zerr);
    if (n < 0 || (zerr != Z_OK && zerr != Z_STREAM_END)) {
        std::cerr << "--with input " << a.with << " is corrupt or truncated: " << (msg ? msg : "") << std::endl;
        gzclose(g);
        return nullptr;
    }
    gzclose(g);
    std::string ext_path = a.with;
    if (gz)
        while (ext_of(ext_path) == ".gz") ext_path = ext_path.substr(0, ext_path.size() - 3);
    const std::string ext = ext_of(ext_path);
    const unsigned char sym = img.empty() ? 0 : img[0];
    int fmt;
    bool ill;
    if (ext == ".fasta" || ext == ".fa") { fmt = KC_FMT_FASTA; ill = sym != '>'; }
    else if (ext == ".fastq" || ext == ".fq") { fmt = KC_FMT_FASTQ; ill = sym != '@'; }
    else { fmt = KC_FMT_PLAIN; ill = !(sym && std::strchr("actgACGT", sym)); }
    if (ill) { std::cerr << "Input file " << a.with << " is ill-formed" << std::endl; return nullptr; }
    kc_chunk* chunks = nullptr;
    uint64_t nch = 0;
    if (kc_plan_chunks(img.data(), img.size(), cfg.k, 0, fmt, &chunks, &nch) != KC_OK) {
        std::cerr << "chunk planning of " << a.with << " failed" << std::endl;
        return nullptr;
    }
    uint64_t staged = 4096;
    for (uint64_t i = 0; i < nch; i++) staged += (chunks[i].len + 4095) / 4096 * 4096;
    cfg.batch_bytes = staged <= (256ull << 20) ? staged : 0;
    kc_ctx* b = nullptr;
    if (kc_create(&cfg, &b) != KC_OK) {
        std::cerr << "kc_create (--with): " << kc_last_error(nullptr) << std::endl;
        kc_free(chunks);
        return nullptr;
    }
    int rc = KC_OK;
    const char* what = "bloom pass";
    if (cfg.bf_enable) {
        for (uint64_t i = 0; i < nch && rc == KC_OK; i++)
            rc = kc_bloom_chunk(b, img.data() + chunks[i].off, chunks[i].len, fmt, chunks[i].broken_header);
        uint64_t nis = 0;
        if (rc == KC_OK) rc = kc_bloom_finalize(b, &nis);
    }
    if (rc == KC_OK) what = "counting pass";
    for (uint64_t i = 0; i < nch && rc == KC_OK; i++)
        rc = kc_count_chunk(b, img.data() + chunks[i].off, chunks[i].len, fmt, chunks[i].broken_header);
    kc_free(chunks);
    if (rc != KC_OK) {
        std::cerr << what << " (--with): " << kc_last_error(b) << std::endl;
        kc_destroy(b);
        return nullptr;
    }
    return b;
}

}  // namespace

int main(int argc, char** argv) {
    Args a;
    int prc = parse(argc, argv, &a);
    if (prc >= 0) return prc;
    std::vector<std::string> qlines;  // --query: read and checked before anything else runs
    std::vector<uint64_t> qkeys;
    if (!a.query.empty() && a.k <= KC_MAX_K) {
        const int qrc = read_queries(a.query, (int)a.k, &qlines, &qkeys);
        if (qrc >= 0) return qrc;
    }
    Coverage cov;  // --coverage: read and checked before anything else runs, too
    if (!a.coverage.empty()) {
        const int crc = read_coverage(a.coverage, &cov);
        if (crc >= 0) return crc;
    }
    Coverage fix;  // --correct: the same
    if (!a.correct.empty()) {
        const int crc = read_coverage(a.correct, &fix, "--correct");
        if (crc >= 0) return crc;
    }
    Coverage thr;  // --paths: likewise
    if (!a.paths.empty()) {
        const int crc = read_coverage(a.paths, &thr, "--paths");
        if (crc >= 0) return crc;
    }

    // ---- format detection (main.cpp:19-68)
    int fd = open(a.input.c_str(), O_RDONLY);
    if (fd < 0) { std::cerr << "cannot open " << a.input << "\n"; return 1; }
    struct stat st;
    fstat(fd, &st);
    const uint64_t fsize = (uint64_t)st.st_size;
    unsigned char magic[2] = {0, 0};
    if (fsize >= 2) { ssize_t r = pread(fd, magic, 2, 0); (void)r; }
    const bool gz = magic[0] == 0x1f && magic[1] == 0x8b;
    std::string ext_path = a.input;
    if (gz) {
        while (ext_of(ext_path) == ".gz") ext_path = ext_path.substr(0, ext_path.size() - 3);
    }
    const std::string ext = ext_of(ext_path);

    // ---- load the image (mmap, or a full gunzip).  The reference's IO thread reads (and inflates)
    // the file and cuts its chunks inside its timers (parallel_parser.hpp:1230-1299,1544-1550): the
    // time of both is added to the first timer line below
    using clk = std::chrono::high_resolution_clock;
    const auto t_in0 = clk::now();
    const uint8_t* image = nullptr;
    uint64_t isize = 0;
    std::vector<uint8_t> gzbuf;
    void* map = nullptr;
    bool bgzf = false;
    if (gz) {  // BGZF: members inflated in parallel
        void* zm = mmap(nullptr, fsize, PROT_READ, MAP_PRIVATE, fd, 0);
        if (zm != MAP_FAILED) {
            const unsigned hw = std::thread::hardware_concurrency();
            bool bad = false;
            bgzf = gunzip_bgzf((const uint8_t*)zm, fsize, (int)std::min(16u, hw ? hw : 1u), &gzbuf, &bad);
            munmap(zm, fsize);
            if (bgzf && bad) {
                std::cerr << "gzip input " << a.input << " is corrupt or truncated: a BGZF member does not inflate"
                          << std::endl;
                return 1;
            }
        }
    }
    if (gz && !bgzf) {
        gzFile g = gzdopen(dup(fd), "r");
        if (!g) { std::cerr << "cannot open " << a.input << " as gzip\n"; return 1; }
        gzbuffer(g, 1 << 20);
        std::vector<uint8_t> tmp(1 << 22);
        int n;
        while ((n = gzread(g, tmp.data(), (unsigned)tmp.size())) > 0) gzbuf.insert(gzbuf.end(), tmp.begin(), tmp.begin() + n);
        int zerr = Z_OK;
        const char* msg = gzerror(g, &zerr);
        // corrupt or truncated stream (zlib reports a cut stream as Z_BUF_ERROR after
        // returning what it decoded): fail instead of counting a prefix
        if (n < 0 || (zerr != Z_OK && zerr != Z_STREAM_END)) {
            std::cerr << "gzip input " << a.input << " is corrupt or truncated: " << (msg ? msg : "") << std::endl;
            gzclose(g);
            return 1;
        }
        gzclose(g);
    }
    if (gz) {
        image = gzbuf.data();
        isize = gzbuf.size();
    } else if (fsize) {
        map = mmap(nullptr, fsize, PROT_READ, MAP_PRIVATE, fd, 0);
        if (map == MAP_FAILED) { std::cerr << "mmap failed\n"; return 1; }
        madvise(map, fsize, MADV_SEQUENTIAL);
        image = (const uint8_t*)map;
        isize = fsize;
    }
    if (!a.gunzip_to.empty()) {  // test hook (tests/test_host.py): the decompressed bytes, no GPU work
        FILE* f = std::fopen(a.gunzip_to.c_str(), "wb");
        if (!f || (isize && std::fwrite(image, 1, isize, f) != isize)) { std::cerr << "cannot write " << a.gunzip_to << "\n"; return 1; }
        std::fclose(f);
        std::cout << "gunzip: " << isize << " bytes" << (bgzf ? " (BGZF, parallel)" : "") << std::endl;
        return 0;
    }
    const unsigned char sym = isize ? image[0] : 0;
    int fmt;
    bool ill = false;
    if (ext == ".fasta" || ext == ".fa") { fmt = KC_FMT_FASTA; ill = sym != '>'; }
    else if (ext == ".fastq" || ext == ".fq") { fmt = KC_FMT_FASTQ; ill = sym != '@'; }
    else { fmt = KC_FMT_PLAIN; ill = !(sym && std::strchr("actgACGT", sym)); }
    if (ill) {
        std::cerr << "Input file " << a.input << " is ill-formed" << std::endl;
        return 1;
    }
    if (a.output.empty()) a.output = stem_of(a.input) + ".kaarme_counts";

    std::cout << "Running settings: " << std::endl;
    std::cout << "  input file:               " << filename_of(a.input) << std::endl;
    std::cout << "  input format:             " << (fmt == KC_FMT_FASTA ? "FASTA" : fmt == KC_FMT_FASTQ ? "FASTQ" : "ONE-STR-PER-LINE") << std::endl;
    std::cout << "  gzip compressed:          " << (gz ? "yes" : "no") << std::endl;
    std::cout << "  k-mer length:             " << a.k << std::endl;
    std::cout << "  min. abundance threshold: " << a.min_abundance << std::endl;
    std::cout << "  hash table type:          " << (a.mode == 0 ? "plain" : "kaarme") << std::endl;
    std::cout << "  using bloom filers:       " << (a.use_bf ? "yes" : "no") << std::endl;
    if (a.use_bf) {
        std::cout << "    est. unique k-mers:     " << a.unique << std::endl;
        std::cout << "    false positive rate:    " << a.fpr << std::endl;
    } else {
        std::cout << "    est. hash table size:   " << a.slots << std::endl;
    }
    std::cout << "  working threads:          " << a.threads << std::endl;
    std::cout << "  output file:              " << a.output << std::endl;
    std::cout << "  device:                   MI355X (HIP device " << a.device << ")" << std::endl;

    if (a.k > KC_MAX_K) {  // fifteen 64-bit key words (include/kc_api.h); INTEGRATION.md "Differences"
        std::cerr << "k-mer length above " << KC_MAX_K << " is not supported by this build" << std::endl;
        return 1;
    }

    const auto t_in1 = clk::now();  // (the input's bytes are in host memory: mapped, or inflated)
    kc_chunk* chunks = nullptr;
    uint64_t nch = 0;
    if (kc_plan_chunks(image, isize, (int)a.k, 0, fmt, &chunks, &nch) != KC_OK) {
        std::cerr << "chunk planning failed" << std::endl;
        return 1;
    }
    const auto t_in2 = clk::now();
    // (an uncompressed file is mapped lazily: its bytes are read by the timed upload, so only the
    // planning counts; a gzip file is inflated here, which the reference does inside its timer)
    const long long prep_us =
        (long long)std::chrono::duration_cast<std::chrono::microseconds>(t_in2 - (gz ? t_in0 : t_in1)).count();

    kc_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.k = (int)a.k;
    cfg.mode = a.mode;
    cfg.bf_enable = a.use_bf;
    cfg.device = a.device;
    cfg.table_slots = a.slots;
    cfg.est_unique = a.unique;
    cfg.fpr = a.fpr;
    cfg.min_abundance = a.min_abundance;
    {   // a small input gets a stage of its own size (one batch, little pinned memory);
        // larger ones the library's default (sized from free HBM)
        uint64_t staged = 4096;
        for (uint64_t i = 0; i < nch; i++) staged += (chunks[i].len + 4095) / 4096 * 4096;
        if (staged <= (256ull << 20)) cfg.batch_bytes = staged;
    }
    kc_ctx* ctx = nullptr;
    if (kc_create(&cfg, &ctx) != KC_OK) {
        std::cerr << "kc_create: " << kc_last_error(nullptr) << std::endl;
        return 1;
    }
    auto die = [&](const char* what) {
        std::cerr << what << ": " << kc_last_error(ctx) << std::endl;
        kc_destroy(ctx);
        std::exit(1);
    };
    // The image goes to HBM once (--host-chunks: stage host chunks instead): both passes
    // then read it in place, and a Bloom job counts from the Bloom pass's partitions
    // (kc_api.h, partition reuse).  Its read is timed with the pass that needs it first,
    // as the reference's reader thread is.  (One reader by default: the C2 sample's timed build
    // 25-28 ms after the warm-up below, against 32-35 ms with two and more with four;
    // profiles/r04_cli_probe_{phases,warmup}.txt)
    const bool host_path = a.host_chunks;
    Upload up;
    const bool staged = !host_path && up.prepare(isize, a.device, a.readers);  // (untimed setup)
    if (staged && !a.no_warmup) {
        // (untimed setup, as the reference's table allocation is) the GPU runtime's one-time
        // work -- loading the counting kernels' code, first launches -- on a one-read input: a
        // -s job on its own context, then kc_reset; a -b job on a small context of its own (a
        // Bloom pass, finalize and the gated pass load the Bloom kernels; the job's context keeps
        // its create-time fine geometry), so the timed passes start on a warm device
        static const char kWarm[] = ">w\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n";
        // the read through the partitioned levels the timed pass takes (a read this short
        // would take the direct path), unless the caller forces a path
        const bool force = std::getenv("KC_INSERT_PATH") == nullptr;
        if (force) setenv("KC_INSERT_PATH", "partitioned", 1);
        uint8_t* dw = nullptr;
        const kc_chunk wc{0, sizeof(kWarm) - 1, 0, 0};
        if (hipMalloc(&dw, sizeof(kWarm)) == hipSuccess) {
            if (hipMemcpy(dw, kWarm, sizeof(kWarm) - 1, hipMemcpyHostToDevice) == hipSuccess) {
                if (!a.use_bf) {
                    if (kc_count_device(ctx, dw, &wc, 1, KC_FMT_FASTA, nullptr) == KC_OK) (void)kc_sync(ctx);
                } else {
                    kc_config w = cfg;
                    w.est_unique = 1000;
                    w.batch_bytes = 1 << 20;
                    kc_ctx* wctx = nullptr;
                    uint64_t nis = 0;
                    if (kc_create(&w, &wctx) == KC_OK && kc_bloom_device(wctx, dw, &wc, 1, KC_FMT_FASTA, nullptr) == KC_OK &&
                        kc_bloom_finalize(wctx, &nis) == KC_OK &&
                        kc_count_device(wctx, dw, &wc, 1, KC_FMT_FASTA, nullptr) == KC_OK)
                        (void)kc_sync(wctx);
                    kc_destroy(wctx);
                }
            }
            (void)hipFree(dw);
        }
        if (force) unsetenv("KC_INSERT_PATH");
        if (!a.use_bf && kc_reset(ctx) != KC_OK) die("reset after warm-up");
    }
    // A -s whose table would take a large share of HBM is sized from the input's distinct estimate
    // inside the timer (below).  Its -s table, allocated by kc_create, is given back first (untimed
    // setup, as the reference's table allocation): beside C5's 192 GB -s table the 10 GB upload
    // crawled at 1.7 GB/s (5.8 s; 0.35 s beside a 96 GB table, profiles/r06_cli_c5_phases.txt)
    const int kw = (int)(a.k / 32 + 1);
    const double s_table_bytes = 1.25 * (double)a.slots / (double)(16 / (kw + 1)) * 128.0;
    const bool want_est = a.table_sizing == 2 || (a.table_sizing == 0 && s_table_bytes > (double)(16ull << 30) && nch > 1);
    bool s_table_dropped = false;
    if (staged && !a.use_bf && want_est) s_table_dropped = kc_size_table(ctx, 1u << 20) == KC_OK;
    uint8_t* d_img = nullptr;
    bool loaded = false;
    auto load = [&]() {
        if (staged && !loaded) {
            loaded = true;
            if (up.run(gz ? -1 : fd, image)) d_img = up.d;
        }
    };
    uint64_t bf_new_in_second = 0;
    if (a.use_bf) {
        std::cout << "Starting parallel bloom filtering\n";
        auto t0 = clk::now();
        load();
        if (d_img) {
            if (kc_bloom_device(ctx, d_img, chunks, nch, fmt, nullptr) != KC_OK) die("bloom pass");
        } else {
            for (uint64_t i = 0; i < nch; i++)
                if (kc_bloom_chunk(ctx, image + chunks[i].off, chunks[i].len, fmt, chunks[i].broken_header) != KC_OK)
                    die("bloom pass");
        }
        uint64_t nis = 0;
        if (kc_bloom_finalize(ctx, &nis) != KC_OK) die("bloom finalize");
        bf_new_in_second = nis;
        auto t1 = clk::now();
        std::cout << "New k-mers in second bloom filter " << nis << "\n";
        std::cout << "Time used to bloom filter k-mers: "
                  << std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count() + prep_us
                  << " microseconds\n";
    }
    std::cout << "Starting " << (a.mode == 0 ? "atomic flag basic" : "atomic variable pointer") << " hash table\n";
    const bool dbg = a.phases;  // phase times on stderr
    auto us = [](clk::time_point x, clk::time_point y) {
        return (long long)std::chrono::duration_cast<std::chrono::microseconds>(y - x).count();
    };
    auto t0 = clk::now();
    // A -s whose table would take a large share of HBM (C4's -s 2.6e9 asks for 83 GB at 25 %
    // headroom; its 1.0 G distinct k-mers need 35 GB) is sized from the whole input's distinct
    // estimate instead (kc_estimate_distinct_device + kc_size_table, inside the timer; -s stays
    // the reference capacity for --strict-capacity), as bench.py's C4 / C5 lines are.  A table
    // that still fills up (an estimate far below the truth) is counted again at -s.
    bool est_sized = false;
    if (staged && !loaded && !a.use_bf && want_est) {
        load();
        double est = 0;
        if (d_img && kc_estimate_distinct_device(ctx, d_img, chunks, nch, fmt, nullptr, &est) == KC_OK) {
            const double want = 1.1 * est + (double)(1 << 20);
            if ((want < 0.8 * (double)a.slots || a.table_sizing == 2) && kc_size_table(ctx, (uint64_t)want) == KC_OK) {
                est_sized = true;
                if (dbg) std::cerr << "cli: table sized from the distinct estimate " << (uint64_t)est << "\n";
            }
        }
    }
    if (s_table_dropped && !est_sized && kc_size_table(ctx, 0) != KC_OK) die("sizing the -s table");
    // A large -s job counts the image's first half while the second half uploads (two counting
    // passes into one table: the second sweeps it once more, ~1.5 ms for C2's, against ~8 ms of
    // the upload hidden); a Bloom job's counting pass follows the Bloom pass, which read it all
    uint64_t split = 0;
    if (staged && !loaded && !a.use_bf && isize >= (512ull << 20) && up.sev.size() && nch > 1) {
        while (split < nch && chunks[split].off + chunks[split].len < isize / 2) split++;
        split = std::min<uint64_t>(split + 1, nch - 1);
    }
    if (split) {
        loaded = true;
        bool up_ok = false;
        std::thread reader([&] { up_ok = up.run(gz ? -1 : fd, image, true); });
        const uint64_t pre_end = chunks[split - 1].off + chunks[split - 1].len + 4096;
        const bool pre_ok = up.wait_prefix(std::min(isize, pre_end));
        const int rc1 = pre_ok ? kc_count_device(ctx, up.d, chunks, split, fmt, nullptr) : KC_OK;
        reader.join();
        up.release();
        if (!pre_ok || !up_ok) {
            up.free_image();
            die("uploading the input");
        }
        if (rc1 != KC_OK) die("counting pass");
        d_img = up.d;
        if (kc_count_device(ctx, d_img, chunks + split, nch - split, fmt, nullptr) != KC_OK) die("counting pass");
        if (dbg) std::cerr << "cli: overlapped upload, counting passes of " << split << " + " << nch - split << " chunks\n";
    } else {
    load();
    auto tl = clk::now();
    if (d_img) {
        if (kc_count_device(ctx, d_img, chunks, nch, fmt, nullptr) != KC_OK) die("counting pass");
        if (dbg) {
            auto tc = clk::now();
            (void)kc_sync(ctx);
            std::cerr << "cli: load " << us(t0, tl) << " us, count call " << us(tl, tc) << " us, its work "
                      << us(tc, clk::now()) << " us\n";
        }
    } else {
        for (uint64_t i = 0; i < nch; i++)
            if (kc_count_chunk(ctx, image + chunks[i].off, chunks[i].len, fmt, chunks[i].broken_header) != KC_OK)
                die("counting pass");
    }
    }
    kc_stats stt;
    int frc = kc_finish(ctx, &stt);
    if (frc == KC_ERR_TABLE_FULL && est_sized) {  // the estimate was too low: the -s table, counted again
        std::cerr << "cli: the estimate-sized table filled up; counting again into the -s table\n";
        if (kc_reset(ctx) != KC_OK || kc_size_table(ctx, 0) != KC_OK ||
            kc_count_device(ctx, d_img, chunks, nch, fmt, nullptr) != KC_OK)
            die("counting pass");
        est_sized = false;
        frc = kc_finish(ctx, &stt);
    }
    if (frc != KC_OK) {
        std::cout << "Hash table is full... Cannot handle this yet\n";
        die("counting pass");
    }
    // --op NAME --with FILE2 (extension): FILE2 counted into a second context, the operation's result
    // into a third -- no Bloom filter, sized from the operands' distinct k-mers -- which everything
    // below (the output, its digest, --histo, --query, --coverage, --correct) then reads instead
    kc_op_stats ost;
    std::memset(&ost, 0, sizeof ost);
    if (a.op >= 0) {
        kc_ctx* ctx_b = count_with(a, cfg);
        if (!ctx_b) { kc_destroy(ctx); return 1; }
        kc_stats stb;
        if (kc_finish(ctx_b, &stb) != KC_OK) {
            std::cerr << "counting pass (--with): " << kc_last_error(ctx_b) << std::endl;
            kc_destroy(ctx_b);
            kc_destroy(ctx);
            return 1;
        }
        const bool uni = a.op == KC_OP_UNION_SUM || a.op == KC_OP_UNION_MAX;
        const uint64_t need = stt.distinct + (uni ? stb.distinct : 0);
        kc_config rcfg = cfg;
        rcfg.bf_enable = 0;
        rcfg.est_unique = 0;
        rcfg.table_slots = need + need / 8 + 4096;
        rcfg.batch_bytes = 1 << 20;  // (nothing is staged into it)
        kc_ctx* ctx_r = nullptr;
        if (kc_create(&rcfg, &ctx_r) != KC_OK) {
            std::cerr << "kc_create (--op): " << kc_last_error(nullptr) << std::endl;
            kc_destroy(ctx_b);
            kc_destroy(ctx);
            return 1;
        }
        kc_op_desc od;
        std::memset(&od, 0, sizeof od);
        od.op = a.op;
        od.a_min = (uint32_t)a.a_min;
        od.a_max = (uint32_t)a.a_max;
        od.b_min = (uint32_t)a.b_min;
        od.b_max = (uint32_t)a.b_max;
        kc_stats str;
        if (kc_table_op(ctx_r, ctx, ctx_b, &od, &ost) != KC_OK || kc_finish(ctx_r, &str) != KC_OK) {
            std::cerr << "table operation " << a.op_name << ": " << kc_last_error(ctx_r) << std::endl;
            kc_destroy(ctx_r);
            kc_destroy(ctx_b);
            kc_destroy(ctx);
            return 1;
        }
        std::cout << "Table operation " << a.op_name << " with " << filename_of(a.with) << ": " << ost.a_keys
                  << " k-mers of the input in range, " << ost.both << " of them in the second file, " << ost.b_only
                  << " only in the second file; result " << ost.out_keys << " k-mers (counts sum " << ost.out_sum
                  << ") in " << str.table_slots << " slots\n";
        kc_destroy(ctx_b);
        kc_destroy(ctx);
        ctx = ctx_r;  // (die reports on it from here on)
    }
    auto t1 = clk::now();
    // the reference prints its table size, next_prime3mod4(-s or 2 * new_in_second)
    // (functions_math.cpp:90); the device table keeps 25 % headroom over it
    const uint64_t ref_slots = kc_table_size_reference(a.use_bf ? 2 * bf_new_in_second : a.slots);
    std::cout << "Hash table size is: " << ref_slots << "\n";
    if (a.min_abundance > 0 && a.digest_only) {
        // --digest-only (extension): the output's order-independent digest (kc_output_digest: lines,
        // sum of T(c), sum and XOR of XXH64 per line) instead of the file -- C4's 60 GB of text
        kc_digest dg;
        if (kc_output_digest(ctx, &dg) != KC_OK) die("output digest");
        char buf[200];
        std::snprintf(buf, sizeof buf, "{\"lines\": %llu, \"count_sum\": %llu, \"hash_sum\": \"%016llx\", \"hash_xor\": \"%016llx\"}",
                      (unsigned long long)dg.lines, (unsigned long long)dg.count_sum, (unsigned long long)dg.hash_sum,
                      (unsigned long long)dg.hash_xor);
        std::cout << "Output digest: " << buf << "\n";
    } else if (a.min_abundance > 0) {
        std::cout << "Start writing k-mers in a file\n";
        if (kc_write(ctx, a.output.c_str()) != KC_OK) die("writing k-mers");
    }
    auto t2 = clk::now();
    if (!a.histo.empty()) {  // extension: the abundance spectrum, every non-zero bin in ascending order
        const uint32_t nb = a.mode == 0 ? 65537 : 16385;
        std::vector<uint64_t> hist(nb);
        if (kc_histogram(ctx, hist.data(), nb) != KC_OK) die("abundance histogram");
        FILE* f = std::fopen(a.histo.c_str(), "w");
        if (!f) { std::cerr << "cannot write " << a.histo << std::endl; kc_destroy(ctx); return 1; }
        for (uint32_t v = 0; v < nb; v++)
            if (hist[v]) std::fprintf(f, "%u %llu\n", v, (unsigned long long)hist[v]);
        if (std::fclose(f) != 0) { std::cerr << "cannot write " << a.histo << std::endl; kc_destroy(ctx); return 1; }
    }
    if (!a.query.empty()) {  // extension: the count of every query line, in order
        std::vector<uint32_t> qcnt(qlines.size());
        if (kc_lookup(ctx, qkeys.data(), qlines.size(), KC_KEYS_DUMP, qcnt.data()) != KC_OK) die("k-mer queries");
        FILE* f = std::fopen(a.query_out.c_str(), "w");
        if (!f) { std::cerr << "cannot write " << a.query_out << std::endl; kc_destroy(ctx); return 1; }
        for (size_t i = 0; i < qlines.size(); i++) std::fprintf(f, "%s %u\n", qlines[i].c_str(), qcnt[i]);
        if (std::fclose(f) != 0) { std::cerr << "cannot write " << a.query_out << std::endl; kc_destroy(ctx); return 1; }
    }
    if (!a.coverage.empty()) {  // extension: the k-mer count statistics of every record, in order
        std::vector<kc_seq_stat> cst(cov.names.size());
        if (kc_seq_stats(ctx, (const uint8_t*)cov.text.data(), cov.text.size(), cov.offsets.data(), cov.names.size(),
                         (uint32_t)a.coverage_min, cst.data()) != KC_OK)
            die("sequence coverage");
        FILE* f = std::fopen(a.coverage_out.c_str(), "w");
        if (!f) { std::cerr << "cannot write " << a.coverage_out << std::endl; kc_destroy(ctx); return 1; }
        for (size_t i = 0; i < cst.size(); i++)
            std::fprintf(f, "%s\t%llu\t%u\t%u\t%u\t%u\t%u\t%u\t%llu\n", cov.names[i].c_str(),
                         (unsigned long long)cov.lengths[i], cst[i].windows, cst[i].present, cst[i].solid, cst[i].min,
                         cst[i].median, cst[i].max, (unsigned long long)cst[i].sum);
        if (std::fclose(f) != 0) { std::cerr << "cannot write " << a.coverage_out << std::endl; kc_destroy(ctx); return 1; }
    }
    if (!a.correct.empty()) {  // extension: the records with their isolated base errors corrected
        const size_t nrec = fix.names.size();
        std::vector<kc_correct_stat> fst(nrec);
        std::string fixed(fix.text.size(), '\0');
        if (kc_correct(ctx, (const uint8_t*)fix.text.data(), fix.text.size(), fix.offsets.data(), nrec,
                       (uint32_t)a.correct_min, (uint8_t*)&fixed[0], fst.data()) != KC_OK)
            die("read correction");
        FILE* f = std::fopen(a.correct_out.c_str(), "w");
        if (!f) { std::cerr << "cannot write " << a.correct_out << std::endl; kc_destroy(ctx); return 1; }
        unsigned long long bases = 0, recs = 0, cands = 0, ambig = 0, dropped = 0;
        for (size_t i = 0; i < nrec; i++) {
            const std::string seq = fixed.substr(fix.offsets[i], fix.lengths[i]);
            if (fix.fmt == KC_FMT_FASTA)
                std::fprintf(f, "%s\n%s\n", fix.headers[i].c_str(), seq.c_str());
            else if (fix.fmt == KC_FMT_FASTQ)
                std::fprintf(f, "%s\n%s\n%s\n%s\n", fix.headers[i].c_str(), seq.c_str(), fix.plus[i].c_str(),
                             fix.quals[i].c_str());
            else
                std::fprintf(f, "%s\n", seq.c_str());
            bases += fst[i].corrected;
            recs += fst[i].corrected != 0;
            cands += fst[i].candidates;
            ambig += fst[i].ambiguous;
            dropped += fst[i].dropped;
        }
        if (std::fclose(f) != 0) { std::cerr << "cannot write " << a.correct_out << std::endl; kc_destroy(ctx); return 1; }
        std::cout << "Corrected " << bases << " bases in " << recs << " of " << nrec << " records (" << cands
                  << " candidates, " << ambig << " ambiguous, " << dropped << " dropped)\n";
    }
    // --clean-tips / --clean-isolated, --pop-bubbles and --cut-weak (extensions): up to --X-rounds rounds of a graph
    // filter, each into a new table sized from a statistics-only call -- no Bloom filter, every k-mer
    // of it output (-a 1) -- which the three graph outputs below read instead of the counted table
    kc_ctx* gctx = ctx;
    auto quit = [&] {
        if (gctx != ctx) kc_destroy(gctx);
        kc_destroy(ctx);
        return 1;
    };
    auto gdie = [&](const char* what) {
        std::cerr << what << ": " << kc_last_error(gctx) << std::endl;
        std::exit(quit());
    };
    // call(dst or nullptr, src, st): the filter; line, say: a round's stats-file and stdout lines; done:
    // the round removed nothing.  false: an error has been reported.
    auto filter_rounds = [&](const FilterOpts& o, const char* what, const char* writing, auto* st, auto call, auto line,
                             auto say, auto done) -> bool {
        auto fail = [](const std::string& where, kc_ctx* of) {
            std::cerr << where << ": " << kc_last_error(of) << std::endl;
            return false;
        };
        FILE* sf = nullptr;
        if (!o.stats.empty() && !(sf = std::fopen(o.stats.c_str(), "w"))) {
            std::cerr << "cannot write " << o.stats << std::endl;
            return false;
        }
        for (unsigned long long round = 1; round <= o.rounds; round++) {
            if (call(nullptr, gctx, st) != KC_OK) return fail(what, gctx);
            kc_config rcfg = cfg;
            rcfg.bf_enable = 0;
            rcfg.est_unique = 0;
            rcfg.min_abundance = 1;
            rcfg.table_slots = st->out_keys + st->out_keys / 8 + 4096;
            rcfg.batch_bytes = 1 << 20;  // (nothing is staged into it)
            kc_ctx* next = nullptr;
            if (kc_create(&rcfg, &next) != KC_OK) return fail(std::string("kc_create (") + what + ")", nullptr);
            kc_stats str;
            if (call(next, gctx, st) != KC_OK || kc_finish(next, &str) != KC_OK) {
                fail(what, next);
                kc_destroy(next);
                return false;
            }
            if (gctx != ctx) kc_destroy(gctx);
            gctx = next;
            if (sf) line(sf, round, *st);
            say(round, *st, str.table_slots);
            if (done(*st)) break;
        }
        if (sf && std::fclose(sf) != 0) {
            std::cerr << "cannot write " << o.stats << std::endl;
            return fail(what, gctx);
        }
        if (!o.out.empty() && kc_write(gctx, o.out.c_str()) != KC_OK) return fail(writing, gctx);
        return true;
    };
    if (a.cleaning()) {
        kc_clean_desc cd;
        std::memset(&cd, 0, sizeof cd);
        cd.min_count = (uint32_t)a.clean.min;
        cd.max_count = (uint32_t)a.clean.max;
        cd.tip_max_nodes = (uint32_t)a.clean_tips;
        cd.iso_max_nodes = (uint32_t)a.clean_iso;
        cd.max_mean = (uint32_t)a.clean.max_mean;
        kc_clean_stats cs;
        if (!filter_rounds(
                a.clean, "graph cleaning", "writing the cleaned k-mers", &cs,
                [&](kc_ctx* dst, kc_ctx* src, kc_clean_stats* st) { return kc_clean(dst, src, &cd, st); },
                [](FILE* sf, unsigned long long round, const kc_clean_stats& cs) {
                    std::fprintf(sf, "round %llu unitigs %llu nodes %llu tips %llu tip_nodes %llu isolated %llu isolated_nodes %llu "
                                     "out_keys %llu out_sum %llu\n", round, (unsigned long long)cs.unitigs,
                                 (unsigned long long)cs.nodes, (unsigned long long)cs.tips, (unsigned long long)cs.tip_nodes,
                                 (unsigned long long)cs.isolated, (unsigned long long)cs.isolated_nodes,
                                 (unsigned long long)cs.out_keys, (unsigned long long)cs.out_sum);
                },
                [](unsigned long long round, const kc_clean_stats& cs, auto slots) {
                    std::cout << "Graph cleaning round " << round << ": " << cs.unitigs << " unitigs, " << cs.nodes
                              << " nodes; removed " << cs.tips << " tips (" << cs.tip_nodes << " nodes) and " << cs.isolated
                              << " isolated unitigs (" << cs.isolated_nodes << " nodes); kept " << cs.out_keys << " k-mers in "
                              << slots << " slots\n";
                },
                [](const kc_clean_stats& cs) { return !cs.tips && !cs.isolated; }))
            return quit();
    }
    // (--pop-bubbles reads the table the cleaning left, or the counted one)
    if (a.pop_set) {
        kc_bubble_desc bd;
        std::memset(&bd, 0, sizeof bd);
        bd.min_count = (uint32_t)a.pop.min;
        bd.max_count = (uint32_t)a.pop.max;
        bd.max_nodes = (uint32_t)a.pop_nodes;
        bd.max_diff = (uint32_t)a.pop_max_diff;
        bd.max_mean = (uint32_t)a.pop.max_mean;
        kc_bubble_stats bs;
        if (!filter_rounds(
                a.pop, "bubble popping", "writing the popped k-mers", &bs,
                [&](kc_ctx* dst, kc_ctx* src, kc_bubble_stats* st) { return kc_pop_bubbles(dst, src, &bd, st); },
                [](FILE* sf, unsigned long long round, const kc_bubble_stats& bs) {
                    std::fprintf(sf, "round %llu unitigs %llu nodes %llu branches %llu parallel %llu popped %llu popped_nodes %llu "
                                     "out_keys %llu out_sum %llu\n", round, (unsigned long long)bs.unitigs,
                                 (unsigned long long)bs.nodes, (unsigned long long)bs.branches, (unsigned long long)bs.parallel,
                                 (unsigned long long)bs.popped, (unsigned long long)bs.popped_nodes,
                                 (unsigned long long)bs.out_keys, (unsigned long long)bs.out_sum);
                },
                [](unsigned long long round, const kc_bubble_stats& bs, auto slots) {
                    std::cout << "Bubble popping round " << round << ": " << bs.unitigs << " unitigs, " << bs.nodes << " nodes, "
                              << bs.branches << " branches, " << bs.parallel << " of them parallel; popped " << bs.popped << " ("
                              << bs.popped_nodes << " nodes); kept " << bs.out_keys << " k-mers in " << slots << " slots\n";
                },
                [](const kc_bubble_stats& bs) { return !bs.popped; }))
            return quit();
    }
    // (--cut-weak reads the table the popping left, or the cleaning, or the counted one)
    if (a.cut_set) {
        kc_weak_desc wd;
        std::memset(&wd, 0, sizeof wd);
        wd.min_count = (uint32_t)a.cut.min;
        wd.max_count = (uint32_t)a.cut.max;
        wd.max_nodes = (uint32_t)a.cut_nodes;
        wd.ratio_permille = (uint32_t)a.cut_ratio;
        wd.max_mean = (uint32_t)a.cut.max_mean;
        kc_weak_stats ws;
        if (!filter_rounds(
                a.cut, "weak-link removal", "writing the cut table's k-mers", &ws,
                [&](kc_ctx* dst, kc_ctx* src, kc_weak_stats* st) { return kc_cut_weak(dst, src, &wd, st); },
                [](FILE* sf, unsigned long long round, const kc_weak_stats& ws) {
                    std::fprintf(sf, "round %llu unitigs %llu nodes %llu interior %llu weak %llu cut %llu cut_nodes %llu "
                                     "out_keys %llu out_sum %llu\n", round, (unsigned long long)ws.unitigs,
                                 (unsigned long long)ws.nodes, (unsigned long long)ws.interior, (unsigned long long)ws.weak,
                                 (unsigned long long)ws.cut, (unsigned long long)ws.cut_nodes,
                                 (unsigned long long)ws.out_keys, (unsigned long long)ws.out_sum);
                },
                [](unsigned long long round, const kc_weak_stats& ws, auto slots) {
                    std::cout << "Weak-link removal round " << round << ": " << ws.unitigs << " unitigs, " << ws.nodes << " nodes, "
                              << ws.interior << " interior, " << ws.weak << " of them weak; cut " << ws.cut << " ("
                              << ws.cut_nodes << " nodes); kept " << ws.out_keys << " k-mers in " << slots << " slots\n";
                },
                [](const kc_weak_stats& ws) { return !ws.cut; }))
            return quit();
    }
    if (!a.graph.empty() || !a.graph_stats.empty()) {  // extension: the de Bruijn graph of the counted (or cleaned, popped) k-mers
        uint64_t* grec = nullptr;
        uint64_t gn = 0;
        kc_graph_stats gst;
        const bool lines = !a.graph.empty();
        if (kc_graph(gctx, (uint32_t)a.graph_min, (uint32_t)a.graph_max, lines ? &grec : nullptr, lines ? &gn : nullptr,
                     &gst) != KC_OK)
            gdie("de Bruijn graph");
        if (lines) {
            FILE* f = std::fopen(a.graph.c_str(), "w");
            if (!f) { std::cerr << "cannot write " << a.graph << std::endl; kc_free(grec); kc_destroy(ctx); return 1; }
            const int W = kc_key_words(gctx), k = (int)a.k;
            std::string line((size_t)k, 'A');
            for (uint64_t i = 0; i < gn; i++) {
                const uint64_t* r = grec + i * (W + 1);
                for (int j = 0; j < k; j++) {  // character j: bits 2(k-1-j).. of the 64 W-bit key
                    const int bit = 2 * (k - 1 - j);
                    line[j] = "ACGT"[(r[W - 1 - bit / 64] >> (bit % 64)) & 3];
                }
                const uint32_t fl = (uint32_t)(r[W] >> 32);
                char e[10];
                for (int y = 0; y < 4; y++) {
                    e[y] = fl & KC_GRAPH_EDGE_R(y) ? "ACGT"[y] : '.';
                    e[5 + y] = fl & KC_GRAPH_EDGE_L(y) ? "ACGT"[y] : '.';
                }
                e[4] = ' ';
                e[9] = '\0';
                std::fprintf(f, "%s %u %s %c%c\n", line.c_str(), (uint32_t)r[W], e, fl & KC_GRAPH_LINK_L ? 'L' : '-',
                             fl & KC_GRAPH_LINK_R ? 'R' : '-');
            }
            kc_free(grec);
            if (std::fclose(f) != 0) { std::cerr << "cannot write " << a.graph << std::endl; kc_destroy(ctx); return 1; }
        }
        const unsigned long long open_unitigs = gst.nodes - gst.link_ends / 2;
        if (!a.graph_stats.empty()) {
            FILE* f = std::fopen(a.graph_stats.c_str(), "w");
            if (!f) { std::cerr << "cannot write " << a.graph_stats << std::endl; kc_destroy(ctx); return 1; }
            std::fprintf(f, "nodes %llu\nedge_ends %llu\nlink_ends %llu\nisolated %llu\npalindromes %llu\n",
                         (unsigned long long)gst.nodes, (unsigned long long)gst.edge_ends, (unsigned long long)gst.link_ends,
                         (unsigned long long)gst.isolated, (unsigned long long)gst.palindromes);
            for (int d = 0; d < 5; d++) std::fprintf(f, "side_degree_%d %llu\n", d, (unsigned long long)gst.side_degree[d]);
            std::fprintf(f, "open_unitigs %llu\n", open_unitigs);
            if (std::fclose(f) != 0) { std::cerr << "cannot write " << a.graph_stats << std::endl; kc_destroy(ctx); return 1; }
        }
        std::cout << "De Bruijn graph: " << gst.nodes << " nodes, " << gst.edge_ends << " edge ends, " << gst.link_ends
                  << " link ends, " << open_unitigs << " open unitigs\n";
    }
    if (!a.unitigs.empty()) {  // extension: the unitigs of that graph, as FASTA
        kc_unitig* urec = nullptr;
        uint8_t* ubases = nullptr;
        kc_unitig_stats ust;
        if (kc_unitigs(gctx, (uint32_t)a.unitigs_min, (uint32_t)a.unitigs_max, &urec, &ubases, &ust) != KC_OK) gdie("unitigs");
        FILE* f = std::fopen(a.unitigs.c_str(), "w");
        if (!f) { std::cerr << "cannot write " << a.unitigs << std::endl; kc_free(urec); kc_free(ubases); kc_destroy(ctx); return 1; }
        char head[160];
        for (uint64_t i = 0; i < ust.unitigs; i++) {
            const kc_unitig& r = urec[i];
            kc::unitig_fasta_header(head, sizeof head, i, r.n_nodes, r.count_sum, (int)a.k, r.flags & KC_UNITIG_CIRCULAR);
            std::fputs(head, f);
            std::fputc('\n', f);
            std::fwrite(ubases + r.offset, 1, (size_t)(r.n_nodes + (uint64_t)a.k - 1), f);
            std::fputc('\n', f);
        }
        kc_free(urec);
        kc_free(ubases);
        if (std::fclose(f) != 0) { std::cerr << "cannot write " << a.unitigs << std::endl; kc_destroy(ctx); return 1; }
        std::cout << "Unitigs: " << ust.unitigs << " (" << ust.circular << " circular), " << ust.nodes << " nodes, "
                  << ust.bases << " bases, longest " << ust.max_nodes << " nodes\n";
    }
    if (!a.gfa.empty()) {  // extension: the compacted graph, unitigs and the edges between them, as GFA 1.0
        kc_unitig* urec = nullptr;
        uint8_t* ubases = nullptr;
        kc_unitig_edge* uedges = nullptr;
        kc_cdbg_stats cst;
        kc_path_run* pruns = nullptr;
        kc_path_stats pst{};
        if (a.paths.empty()) {
            if (kc_unitig_graph(gctx, (uint32_t)a.gfa_min, (uint32_t)a.gfa_max, &urec, &ubases, &uedges, &cst) != KC_OK) gdie("gfa");
        } else if (kc_read_paths(gctx, (uint32_t)a.gfa_min, (uint32_t)a.gfa_max, &urec, &ubases, &uedges, &cst,
                                 (const uint8_t*)thr.text.data(), thr.text.size(), thr.offsets.data(), thr.names.size(),
                                 &pruns, nullptr, &pst) != KC_OK) {
            gdie("paths");
        }
        FILE* f = std::fopen(a.gfa.c_str(), "w");
        if (!f) {
            std::cerr << "cannot write " << a.gfa << std::endl;
            kc_free(urec); kc_free(ubases); kc_free(uedges); kc_free(pruns); kc_destroy(ctx);
            return 1;
        }
        const unsigned long long ov = (unsigned long long)a.k - 1;
        std::fputs("H\tVN:Z:1.0\n", f);
        for (uint64_t i = 0; i < cst.unitigs; i++) {
            const kc_unitig& r = urec[i];
            const uint64_t len = r.n_nodes + ov;
            std::fprintf(f, "S\t%llu\t", (unsigned long long)i);
            std::fwrite(ubases + r.offset, 1, (size_t)len, f);
            std::fprintf(f, "\tLN:i:%llu\tKC:i:%llu\n", (unsigned long long)len, (unsigned long long)r.count_sum);
        }
        for (uint64_t j = 0; j < cst.edges; j++) {
            const kc_unitig_edge& e = uedges[j];
            std::fprintf(f, "L\t%u\t%c\t%u\t%c\t%lluM\n", e.from, e.flags & KC_EDGE_FROM_REV ? '-' : '+', e.to,
                         e.flags & KC_EDGE_TO_REV ? '-' : '+', ov);
        }
        for (uint64_t i = 0; i < cst.unitigs; i++)  // a circle's closing link, on either strand
            if (urec[i].flags & KC_UNITIG_CIRCULAR)
                std::fprintf(f, "L\t%llu\t+\t%llu\t+\t%lluM\nL\t%llu\t-\t%llu\t-\t%lluM\n", (unsigned long long)i,
                             (unsigned long long)i, ov, (unsigned long long)i, (unsigned long long)i, ov);
        bool paths_ok = true;
        if (!a.paths.empty()) {  // the runs as GAF, a line per chain in run order
            FILE* g = std::fopen(a.paths_out.c_str(), "w");
            paths_ok = g != nullptr;
            kc::GafPath gp;
            uint64_t chain_seq = 0, qstart = 0;
            auto flush = [&] {
                if (!gp.visits) return;
                const unsigned long long aln = gp.pend - gp.pstart;
                std::fprintf(g, "%s\t%llu\t%llu\t%llu\t+\t%s\t%llu\t%llu\t%llu\t%llu\t%llu\t255\tcg:Z:%llu=\n",
                             thr.names[chain_seq].c_str(), (unsigned long long)thr.lengths[chain_seq],
                             (unsigned long long)qstart, (unsigned long long)qstart + aln, gp.path.c_str(),
                             (unsigned long long)gp.plen, (unsigned long long)gp.pstart, (unsigned long long)gp.pend, aln, aln, aln);
                gp = kc::GafPath{};
            };
            for (uint64_t j = 0; g && j < pst.runs; j++) {
                const kc_path_run& r = pruns[j];
                if (!(r.flags & KC_RUN_JOINED)) {
                    flush();
                    chain_seq = r.seq;
                    qstart = r.text_pos - thr.offsets[r.seq];
                }
                const kc_unitig& u = urec[r.unitig];
                kc::gaf_add_run(gp, r.unitig, r.flags & KC_RUN_REV, r.pos, r.windows, u.n_nodes, u.flags & KC_UNITIG_CIRCULAR,
                                (int)a.k);
            }
            if (g) {
                flush();
                if (std::fclose(g) != 0) paths_ok = false;
            }
            if (!paths_ok) std::cerr << "cannot write " << a.paths_out << std::endl;
            if (paths_ok && !a.paths_stats.empty()) {
                FILE* h = std::fopen(a.paths_stats.c_str(), "w");
                if (h)
                    std::fprintf(h, "seqs %llu\nwindows %llu\nlocated %llu\nruns %llu\nchains %llu\nthreaded %llu\n",
                                 (unsigned long long)pst.seqs, (unsigned long long)pst.windows, (unsigned long long)pst.located,
                                 (unsigned long long)pst.runs, (unsigned long long)pst.chains, (unsigned long long)pst.threaded);
                if (!h || std::fclose(h) != 0) {
                    std::cerr << "cannot write " << a.paths_stats << std::endl;
                    paths_ok = false;
                }
            }
        }
        kc_free(urec);
        kc_free(ubases);
        kc_free(uedges);
        kc_free(pruns);
        if (std::fclose(f) != 0) { std::cerr << "cannot write " << a.gfa << std::endl; kc_destroy(ctx); return 1; }
        if (!paths_ok) { kc_destroy(ctx); return 1; }
        if (!a.paths.empty())
            std::cout << "Read paths: " << pst.seqs << " sequences, " << pst.windows << " k-mers, " << pst.located
                      << " located, " << pst.runs << " runs, " << pst.chains << " chains, " << pst.threaded
                      << " threaded whole\n";
        std::cout << "Compacted graph: " << cst.unitigs << " unitigs (" << cst.circular << " circular), " << cst.nodes
                  << " nodes, " << cst.bases << " bases, longest " << cst.max_nodes << " nodes, " << cst.edges
                  << " edges, " << cst.dead_ends << " dead ends\n";
    }
    auto t3 = clk::now();
    std::cout << "Time used to build hash table: "
              << std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count() + (a.use_bf ? 0 : prep_us)
              << " microseconds\n";
    std::cout << "Input read and chunked in " << prep_us << " microseconds (included in the first timer line)\n";
    if (est_sized)
        std::cout << "Device table sized from the distinct estimate (-s " << a.slots
                  << " stays the reference capacity)\n";
    std::cout << "Time used to write k-mers in a file: "
              << std::chrono::duration_cast<std::chrono::microseconds>(t2 - t1).count() << " microseconds\n";
    if (!a.histo.empty() || !a.query.empty() || !a.coverage.empty() || !a.correct.empty() || !a.graph.empty() ||
        !a.graph_stats.empty() || !a.unitigs.empty() || !a.gfa.empty() || a.cleaning() || a.pop_set || a.cut_set)
        std::cout << "Time used to query the hash table: "
                  << std::chrono::duration_cast<std::chrono::microseconds>(t3 - t2).count() << " microseconds"
                  << (a.query.empty() ? "" : " (" + std::to_string(qlines.size()) + " queries)")
                  << (a.coverage.empty() ? "" : " (" + std::to_string(cov.names.size()) + " coverage records)") << "\n";
    std::cout << "Processed k-mers: " << stt.windows << " (inserted " << stt.inserted << ")\n";
    std::cout << "Main array slots used " << stt.distinct << " / " << ref_slots << "\n";
    std::cout << "Device table capacity: " << stt.table_slots << " slots\n";
    std::cout << "Input path: " << (d_img ? "device image" : "host chunks")
              << (stt.reused_passes ? " (counting pass from the Bloom pass's partitions)" : "") << "\n";
    if (gctx != ctx) kc_destroy(gctx);
    kc_destroy(ctx);
    up.release();
    up.free_image();
    kc_free(chunks);
    if (map) munmap(map, fsize);
    close(fd);
    return 0;
}
