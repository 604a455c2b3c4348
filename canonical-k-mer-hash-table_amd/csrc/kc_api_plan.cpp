// kc_api_plan.cpp -- entry points that need no context: the chunk planner, the device XXH64 test
// hook and the synthetic read generator (include/kc_api.h).
#include "kc_ctx.h"
#include "kc_synth.h"

// The chunk planner reads the image only around chunk ends (io_worker / read_chunk_from_file,
// parallel_parser.hpp:1246-1285, text_reader.h:93-226): templated over how bytes are read --
// a host pointer, or 64 KiB pages of a device image fetched on demand (kc_plan_chunks_device:
// a 1.6 GB image costs its ~160 chunk ends, not a copy of the image)
struct HostImg {
    const uint8_t* p;
    uint8_t operator[](uint64_t i) const { return p[i]; }
    uint64_t find(uint64_t from, uint8_t c, uint64_t size) const {  // first c at >= from, or size
        const void* q = std::memchr(p + from, c, size - from);
        return q ? (uint64_t)((const uint8_t*)q - p) : size;
    }
};

struct DeviceImg {
    static constexpr uint64_t PAGE = 64 << 10;
    const uint8_t* d;
    uint64_t size;
    std::vector<std::pair<uint64_t, std::vector<uint8_t>>> cache;  // a few pages, most recent last
    bool bad = false;
    uint64_t fetched = 0;
    const std::vector<uint8_t>& page(uint64_t pg) {
        for (size_t i = 0; i < cache.size(); i++)
            if (cache[i].first == pg) return cache[i].second;
        if (cache.size() >= 8) cache.erase(cache.begin());
        const uint64_t off = pg * PAGE, len = std::min(PAGE, size - off);
        std::vector<uint8_t> buf(len);
        if (hipMemcpy(buf.data(), d + off, len, hipMemcpyDeviceToHost) != hipSuccess) bad = true;
        fetched += len;
        cache.emplace_back(pg, std::move(buf));
        return cache.back().second;
    }
    uint8_t operator[](uint64_t i) { return page(i / PAGE)[i % PAGE]; }
    uint64_t find(uint64_t from, uint8_t c, uint64_t sz) {
        while (from < sz) {
            const auto& pg = page(from / PAGE);
            const uint64_t o = from % PAGE;
            const void* q = std::memchr(pg.data() + o, c, pg.size() - o);
            if (q) return from - o + (uint64_t)((const uint8_t*)q - pg.data());
            from += pg.size() - o;
        }
        return sz;
    }
};

template <class Img>
static int plan_chunks_impl(Img& image, uint64_t size, int k, uint64_t chunk_size, int fmt, kc_chunk** out,
                            uint64_t* n_out) {
    if (chunk_size == 0) chunk_size = 10ull << 20;  // main.cpp:387
    std::vector<kc_chunk> v;
    if (fmt == KC_FMT_FASTQ) {
        // FASTQ (extension; the reference rejects it): chunks of whole 4-line records, no
        // overlap (a k-mer never spans records).  A record starts at a line that begins
        // with '@' and whose second next line begins with '+' (a quality line starting
        // with '@' is followed two lines later by a sequence line, never by '+').
        auto line_after = [&](uint64_t p) -> uint64_t {  // start of the line after the one at p
            const uint64_t q = image.find(p, '\n', size);
            return q < size ? q + 1 : size;
        };
        auto is_record = [&](uint64_t p) {
            if (p >= size || image[p] != '@') return false;
            const uint64_t l2 = line_after(line_after(p));
            return l2 < size && image[l2] == '+';
        };
        uint64_t pos = 0;
        while (pos < size) {
            uint64_t end = size;
            if (size - pos > chunk_size) {
                end = 0;
                // last record start in (pos, pos + chunk_size]: walk back over line starts
                for (uint64_t q = pos + chunk_size; q > pos; q--)
                    if (image[q - 1] == '\n' && is_record(q)) { end = q; break; }
                if (!end) {  // one record longer than a chunk: cut after it
                    end = size;
                    for (uint64_t q = line_after(pos); q < size; q = line_after(q))
                        if (is_record(q)) { end = q; break; }
                }
            }
            v.push_back(kc_chunk{pos, end - pos, 0, 0});
            pos = end;
        }
    } else {
    const unsigned char start = fmt == KC_FMT_FASTA ? '>' : 0;
    // io_worker: loop while rem >= k, each chunk min(chunk_size, rem) bytes, then
    // read_chunk_from_file with its k = k-1 (parallel_parser.hpp:1246-1285).
    const int64_t back = (int64_t)k - 1;
    int64_t rem = (int64_t)size;
    uint64_t pos = 0;
    bool bh = false;
    while (rem >= (int64_t)k) {
        const int64_t n = std::min<int64_t>((int64_t)chunk_size, rem);
        auto b = [&](int64_t i) { return image[pos + (uint64_t)i]; };
        kc_chunk ck{pos, (uint64_t)n, bh ? 1 : 0, 0};
        v.push_back(ck);
        int64_t fake = 0;
        if (start) {
            int64_t real = 0, si = n - 1;
            if (start == '>')
                for (; real < back && si >= 0; si--) (b(si) != '\n') ? real++ : fake++;  // text_reader.h:143-150
            if (real != back) break;                                                 // text_reader.h:156-160
            // broken header of the NEXT chunk: scan back from the byte before its start
            bh = true;
            for (int64_t i = n - 1 - back - fake; i >= 0; i--) {  // text_reader.h:164-184
                if (b(i) == start) break;
                if (b(i) == '\n') { bh = false; break; }
            }
        }
        if (rem == n) break;                 // text_reader.h:201-204
        const int64_t adv = n - back - fake;  // seek back (k-1) + fake (text_reader.h:210-220)
        if (adv == 0) break;
        rem -= adv;
        pos += (uint64_t)adv;
    }
    }
    kc_chunk* r = (kc_chunk*)std::malloc(std::max<size_t>(1, v.size()) * sizeof(kc_chunk));
    if (!r) return KC_ERR_NOMEM;
    if (!v.empty()) std::memcpy(r, v.data(), v.size() * sizeof(kc_chunk));
    *out = r;
    *n_out = v.size();
    return KC_OK;
}

extern "C" {

int kc_plan_chunks(const uint8_t* image, uint64_t size, int k, uint64_t chunk_size, int fmt, kc_chunk** out,
                   uint64_t* n_out) {
    if (!out || !n_out || k < 1 || (!image && size)) return KC_ERR_ARG;
    HostImg img{image};
    return plan_chunks_impl(img, size, k, chunk_size, fmt, out, n_out);
}

int kc_plan_chunks_device(const uint8_t* dev_image, uint64_t size, int k, uint64_t chunk_size, int fmt, kc_chunk** out,
                          uint64_t* n_out) {
    if (!out || !n_out || k < 1 || (!dev_image && size)) return KC_ERR_ARG;
    if (hipDeviceSynchronize() != hipSuccess) return KC_ERR_HIP;  // the image's producers are done
    DeviceImg img{dev_image, size, {}};
    const int rc = plan_chunks_impl(img, size, k, chunk_size, fmt, out, n_out);
    if (rc == KC_OK && img.bad) {
        std::free(*out);
        *out = nullptr;
        *n_out = 0;
        return KC_ERR_HIP;
    }
    return rc;
}

int kc_xxh64(const uint64_t* values, const uint64_t* seeds, uint64_t n, uint64_t* out) {
    if (n && (!values || !seeds || !out)) return KC_ERR_ARG;
    if (n == 0) return KC_OK;
    DevBuf<uint64_t> d;
    if (!d.reserve(n * 3)) return KC_ERR_NOMEM;
    hipError_t e = hipMemcpy(d, values, n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, seeds, n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_xxh64(d, d + n, n, d + 2 * n, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d + 2 * n, n * 8, hipMemcpyDeviceToHost);
    return e == hipSuccess ? KC_OK : KC_ERR_HIP;
}

uint64_t kc_synth_bytes(uint64_t first_read, uint64_t n_reads, uint32_t read_len, uint32_t wrap) {
    kc_synth_params p{};
    p.read_len = read_len;
    p.wrap = wrap;
    return kcs_record_offset(&p, first_read + n_reads) - kcs_record_offset(&p, first_read);
}

int kc_synth_device(uint8_t* dst, uint64_t first_read, uint64_t n_reads, uint64_t seed, uint64_t genome_len,
                    uint32_t read_len, uint32_t wrap, double err_rate, double n_rate, void* s) {
    if (!dst || genome_len < read_len || read_len == 0) return KC_ERR_ARG;
    hipError_t e = launch_synth(dst, first_read, n_reads, seed, genome_len, read_len, wrap, err_rate, n_rate,
                                nullptr, (hipStream_t)s);
    return e == hipSuccess ? KC_OK : KC_ERR_HIP;
}

int kc_synth_skew_device(uint8_t* dst, uint64_t first_read, uint64_t n_reads, uint64_t seed, uint64_t genome_len,
                         uint32_t read_len, uint32_t wrap, double err_rate, double n_rate, const kc_synth_skew* skew,
                         void* s) {
    if (!dst || genome_len < read_len || read_len == 0) return KC_ERR_ARG;
    hipError_t e = launch_synth(dst, first_read, n_reads, seed, genome_len, read_len, wrap, err_rate, n_rate, skew,
                                (hipStream_t)s);
    return e == hipSuccess ? KC_OK : KC_ERR_HIP;
}

}  // extern "C"
