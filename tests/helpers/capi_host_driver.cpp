// capi_host_driver.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program over the host data path of afsk_capi.hip,
// linked statically with it, the stub launchers and the fake HIP runtime (build_stub_lib.sh <program> -fsanitize=...),
// so that ThreadSanitizer / AddressSanitizer see the staging ring's hand-over without any interpreter in the process.
// "Device" memory is host memory.  With a ring of 3 x 4 MiB and 6 I/O threads it
//   1. writes canonical files through afsk_wav_egress from a buffer of several times the ring's size (one stream longer
//      than a window, one exactly a window, empty streams, gaps on both sides of 64 KiB) and checks every file's bytes,
//   2. reads them back through afsk_wav_ingest and through afsk_wav_probe + afsk_wav_upload (gaps on both sides of
//      256 B) and checks every sample, the zero fill and what must stay untouched,
//   3. calls afsk_demod_streams_host from four threads at once.
// Exit status 0 = everything matched; 1 = a mismatch or a failed call (named on stderr).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "../../include/afsk_amd.h"

namespace {

int g_bad = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        if (!(cond)) {                                                         \
            if (g_bad++ < 20) { std::fprintf(stderr, "MISMATCH %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } \
        }                                                                      \
    } while (0)

constexpr int16_t kPattern = 0x5A5A;

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_rng >> 33); }

std::vector<unsigned char> read_file(const std::string& fn) {
    std::vector<unsigned char> out;
    if (FILE* f = std::fopen(fn.c_str(), "rb")) {
        unsigned char buf[1 << 16];
        size_t r;
        while ((r = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + r);
        std::fclose(f);
    }
    return out;
}

// what the stdlib writer emits for 1 channel / 16 bit / 48000 Hz, written out independently of the library
void expected_header(unsigned char* h, uint32_t data_bytes) {
    auto p32 = [](unsigned char* q, uint32_t v) { for (int k = 0; k < 4; k++) q[k] = (unsigned char)(v >> (8 * k)); };
    std::memcpy(h, "RIFF", 4); p32(h + 4, 36 + data_bytes); std::memcpy(h + 8, "WAVEfmt ", 8); p32(h + 16, 16);
    h[20] = 1; h[21] = 0; h[22] = 1; h[23] = 0; p32(h + 24, 48000); p32(h + 28, 96000);
    h[32] = 2; h[33] = 0; h[34] = 16; h[35] = 0; std::memcpy(h + 36, "data", 4); p32(h + 40, data_bytes);
}

// a layout: slot s of `slot[s]` samples at off[s], gaps (in samples) drawn from `gaps` in turn
std::vector<int64_t> lay_out(const std::vector<int64_t>& slot, const std::vector<int64_t>& gaps, std::vector<int64_t>* gap_behind) {
    std::vector<int64_t> off(slot.size());
    gap_behind->assign(slot.size(), 0);
    int64_t at = 0;
    for (size_t s = 0; s < slot.size(); s++) {
        off[s] = at;
        (*gap_behind)[s] = gaps[(s * 7 + 3) % gaps.size()];
        at += slot[s] + (*gap_behind)[s];
    }
    return off;
}

// dev[off[s] ...] holds stream s, `fill` samples behind it are zero (its slot's rest and a small gap), all else is untouched
void check_delivery(const char* what, const std::vector<int16_t>& dev, const std::vector<int16_t>& src,
                    const std::vector<int64_t>& src_off, const std::vector<int32_t>& len, const std::vector<int64_t>& off,
                    const std::vector<int64_t>& zero_behind) {
    std::vector<char> covered(dev.size(), 0);
    for (size_t s = 0; s < len.size(); s++) {
        CHECK(std::memcmp(dev.data() + off[s], src.data() + src_off[s], (size_t)len[s] * 2) == 0, "%s: stream %zu differs", what, s);
        bool zeros = true;
        for (int64_t k = 0; k < zero_behind[s]; k++) zeros = zeros && dev[(size_t)(off[s] + len[s] + k)] == 0;
        CHECK(zeros, "%s: the %lld samples behind stream %zu are not all zero", what, (long long)zero_behind[s], s);
        std::memset(covered.data() + off[s], 1, (size_t)(len[s] + zero_behind[s]));
    }
    size_t touched = 0;
    for (size_t k = 0; k < dev.size(); k++) touched += !covered[k] && dev[k] != kPattern;
    CHECK(touched == 0, "%s: %zu samples outside every slot were written", what, touched);
}

}  // namespace

int main(int argc, char** argv) {
    setenv("AFSK_INGEST_WINDOW_MB", "4", 1);         // read by the library on its first file entry
    setenv("AFSK_INGEST_SLOTS", "3", 1);
    setenv("AFSK_IO_THREADS", "6", 1);
    std::string dir = argc > 1 ? argv[1] : "";
    if (dir.empty()) {
        const char* t = std::getenv("TMPDIR");
        std::string tmpl = std::string(t && *t ? t : "/tmp") + "/capi_host_driver.XXXXXX";
        if (!mkdtemp(&tmpl[0])) { std::perror("mkdtemp"); return 1; }
        dir = tmpl;
    }
    if (afsk_device_count() != 1) { std::fprintf(stderr, "not the fake runtime\n"); return 1; }

    // ---- the streams: 40 of them, ~52 MB = four times the ring
    const int64_t kWindowSamples = (4 << 20) / 2;
    const std::vector<int64_t> shape = {0, 1, 48000, 3000001, 5, 0, 700000, kWindowSamples, 48000, 333,
                                        1500000, 0, 900001, 2500000, 96000, 7, 1200000, 48000, 0, 2097151};
    std::vector<int32_t> len;
    for (int rep = 0; rep < 2; rep++)
        for (int64_t v : shape) len.push_back((int32_t)(v + (v > 1000 ? (int64_t)(rnd() % 64) * rep : 0)));
    const int32_t n = (int32_t)len.size();
    // gaps in samples: none, small, 65534 / 65536 / 65538 B (egress copies a gap of up to 64 KiB along), large
    std::vector<int64_t> e_gap;
    const std::vector<int64_t> e_off = lay_out(std::vector<int64_t>(len.begin(), len.end()), {0, 8, 32767, 32768, 32769, 100000, 0, 300}, &e_gap);
    const size_t e_total = (size_t)(e_off[n - 1] + len[n - 1]) + 100;
    std::vector<int16_t> src(e_total);
    for (int16_t& v : src) v = (int16_t)rnd();

    std::vector<std::string> names;
    std::vector<const char*> paths;
    for (int32_t s = 0; s < n; s++) names.push_back(dir + "/d" + std::to_string(s) + ".wav");
    for (const std::string& fn : names) paths.push_back(fn.c_str());

    // ---- 1. egress, twice (the second call overwrites in place; the ring's buffers and events are reused across calls)
    for (int rep = 0; rep < 2; rep++) {
        std::vector<int32_t> status(n, -7);
        const int rc = afsk_wav_egress(paths.data(), n, src.data(), e_off.data(), len.data(), status.data());
        CHECK(rc == AFSK_OK, "afsk_wav_egress returned %d", rc);
        for (int32_t s = 0; s < n; s++) {
            CHECK(status[s] == AFSK_WAV_OK, "egress status[%d] = %d", s, status[s]);
            const std::vector<unsigned char> got = read_file(names[s]);
            unsigned char hdr[44];
            expected_header(hdr, (uint32_t)len[s] * 2u);
            CHECK(got.size() == 44 + (size_t)len[s] * 2 && std::memcmp(got.data(), hdr, 44) == 0 &&
                  std::memcmp(got.data() + 44, src.data() + e_off[s], (size_t)len[s] * 2) == 0, "egress: file %d differs", s);
        }
    }

    // ---- 2a. one-pass ingest into slots of a multiple of 8 samples; gaps of 252 / 256 B travel as zeros, 260 B and more do not
    {
        std::vector<int64_t> slot(n), gap, zero_behind(n);
        for (int32_t s = 0; s < n; s++) slot[s] = ((int64_t)len[s] + 7) & ~(int64_t)7;
        const std::vector<int64_t> off = lay_out(slot, {0, 8, 126, 128, 130, 4096, 64, 0}, &gap);
        for (int32_t s = 0; s < n; s++) zero_behind[s] = slot[s] - len[s] + (s + 1 < n && gap[s] <= 128 ? gap[s] : 0);
        const int64_t total = off[n - 1] + slot[n - 1] + 1000;
        for (int rep = 0; rep < 2; rep++) {
            std::vector<int16_t> dev((size_t)total, kPattern);
            std::vector<int64_t> d_off(n), d_bytes(n);
            std::vector<int32_t> status(n, -7);
            const int rc = afsk_wav_ingest(paths.data(), n, off.data(), slot.data(), dev.data(), total, d_off.data(), d_bytes.data(), status.data());
            CHECK(rc == AFSK_OK, "afsk_wav_ingest returned %d", rc);
            for (int32_t s = 0; s < n; s++)
                CHECK(status[s] == AFSK_WAV_OK && d_off[s] == 44 && d_bytes[s] == (int64_t)len[s] * 2, "ingest: file %d: status %d, %lld bytes at %lld",
                      s, status[s], (long long)d_bytes[s], (long long)d_off[s]);
            check_delivery("ingest", dev, src, e_off, len, off, zero_behind);
        }
    }

    // ---- 2b. probe + upload (the two-window loop), unaligned streams
    {
        std::vector<int64_t> d_off(n), d_bytes(n), gap, zero_behind(n);
        std::vector<int32_t> status(n, -7);
        int rc = afsk_wav_probe(paths.data(), n, d_off.data(), d_bytes.data(), status.data());
        CHECK(rc == AFSK_OK, "afsk_wav_probe returned %d", rc);
        for (int32_t s = 0; s < n; s++)
            CHECK(status[s] == AFSK_WAV_OK && d_off[s] == 44 && d_bytes[s] == (int64_t)len[s] * 2, "probe: file %d", s);
        const std::vector<int64_t> off = lay_out(std::vector<int64_t>(len.begin(), len.end()), {0, 3, 7, 128, 129, 5000}, &gap);
        for (int32_t s = 0; s < n; s++) zero_behind[s] = s + 1 < n && gap[s] <= 128 ? gap[s] : 0;
        const int64_t total = off[n - 1] + len[n - 1] + 64;
        std::vector<int16_t> dev((size_t)total, kPattern);
        rc = afsk_wav_upload(paths.data(), d_off.data(), d_bytes.data(), off.data(), n, dev.data(), total);
        CHECK(rc == AFSK_OK, "afsk_wav_upload returned %d", rc);
        check_delivery("upload", dev, src, e_off, len, off, zero_behind);
    }

    // ---- 3. the gather entry from four threads at once (one shared scratch cache, the pinned windows, per-thread streams)
    {
        std::vector<std::thread> th;
        std::vector<int> rcs(4, -1);
        for (int k = 0; k < 4; k++)
            th.emplace_back([&, k] {
                int worst = AFSK_OK;
                for (int rep = 0; rep < 3; rep++) {
                    const int32_t m = 24 + 5 * k + rep;
                    std::vector<const int16_t*> streams(m);
                    std::vector<int32_t> ln(m), bf(m), out[5];
                    for (int32_t s = 0; s < m; s++) {
                        ln[s] = (int32_t)((uint32_t)(s * 7919 + k * 104729 + rep * 31) % 400000u);
                        streams[s] = src.data() + (size_t)(s * 1000003 + k * 17) % (e_total - 400000);
                        bf[s] = (k & 1) && s % 3 == 0 ? 160 : 40;
                    }
                    for (auto& o : out) o.assign(m, 0);
                    std::vector<uint8_t> bytes((size_t)m * 8);
                    const int rc = afsk_demod_streams_host(streams.data(), ln.data(), bf.data(), 14000, m, bytes.data(), 8, out[0].data(),
                                                           out[1].data(), out[2].data(), out[3].data(), out[4].data());
                    if (rc != AFSK_OK) worst = rc;
                }
                rcs[k] = worst;
            });
        for (std::thread& t : th) t.join();
        for (int k = 0; k < 4; k++) CHECK(rcs[k] == AFSK_OK, "afsk_demod_streams_host, thread %d: %d", k, rcs[k]);
    }
    CHECK(afsk_host_scratch_release() == AFSK_OK, "afsk_host_scratch_release");

    for (const std::string& fn : names) unlink(fn.c_str());
    if (argc <= 1) rmdir(dir.c_str());
    if (g_bad) { std::fprintf(stderr, "capi_host_driver: %d mismatches\n", g_bad); return 1; }
    std::printf("capi_host_driver OK: %d files, %.1f MB through a 3 x 4 MiB ring\n", n, (double)e_total * 2e-6);
    return 0;
}
