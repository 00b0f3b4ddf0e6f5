// afsk_host_riff.h -- what the host entries know about RIFF/WAVE files: little-endian fields, the chunk walk of
// the stdlib reader, and the canonical 44-byte header ('RIFF' size 'WAVE' 'fmt ' 16 ... 'data' size) both ways.
// Host code only, included by afsk_capi.hip alone (everything here has internal linkage).
#pragma once

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/afsk_amd.h"

namespace {

bool pread_all(int fd, void* dst, size_t bytes, int64_t off) {
    char* p = (char*)dst;
    while (bytes > 0) {
        const ssize_t r = pread(fd, p, bytes, (off_t)off);
        if (r <= 0) return false;
        p += r; off += r; bytes -= (size_t)r;
    }
    return true;
}

uint32_t le32(const unsigned char* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
uint32_t le16(const unsigned char* p) { return p[0] | (p[1] << 8); }
void put_le32(unsigned char* q, uint32_t v) { q[0] = (unsigned char)v; q[1] = (unsigned char)(v >> 8); q[2] = (unsigned char)(v >> 16); q[3] = (unsigned char)(v >> 24); }
void put_le16(unsigned char* q, uint32_t v) { q[0] = (unsigned char)v; q[1] = (unsigned char)(v >> 8); }

// The chunk walk of Python's wave.Wave_read.initfp + chunk.Chunk (what ref:214 runs), without
// interpreting the audio format: returns AFSK_WAV_* and the byte range readframes(getnframes()) covers.
// On an open file (the caller closes it).
int wav_probe_fd(int fd, int64_t* data_off, int64_t* data_bytes) {
    *data_off = 0; *data_bytes = 0;
    // ONE read covers the RIFF header and the chunk headers of nearly every file (44-byte header,
    // perhaps a LIST chunk); chunk headers beyond it are read one by one.  The file size comes from
    // a short read or, for longer files, from fstat.
    constexpr int64_t kHead = 512;
    unsigned char head[kHead];
    int64_t have = 0;
    for (;;) {
        const ssize_t r = pread(fd, head + have, (size_t)(kHead - have), (off_t)have);
        if (r < 0) return AFSK_WAV_IO;
        if (r == 0) break;
        have += r;
        if (have == kHead) break;
    }
    int64_t fsize = have;
    if (have == kHead) {
        struct stat st;
        if (fstat(fd, &st) != 0) return AFSK_WAV_IO;
        fsize = (int64_t)st.st_size;
    }
    auto fetch = [&](int64_t off, int n, unsigned char* dst) {      // n bytes at off, from the buffer when possible
        if (off + n <= have) { std::memcpy(dst, head + off, (size_t)n); return true; }
        return pread_all(fd, dst, (size_t)n, off);
    };
    unsigned char h[16];
    int rc = AFSK_WAV_NO_DATA;
    if (fsize < 12 || std::memcmp(head, "RIFF", 4) != 0 || std::memcmp(head + 8, "WAVE", 4) != 0)
        return AFSK_WAV_NOT_RIFF;
    // chunks inside the RIFF form end where the RIFF size says (Chunk.read clips to it), or at EOF
    const int64_t form_end = std::min<int64_t>(fsize, 8 + (int64_t)le32(head + 4));
    int64_t pos = 12;
    int64_t framesize = 0;
    while (pos + 8 <= form_end) {
        if (!fetch(pos, 8, h)) { rc = AFSK_WAV_IO; break; }
        const int64_t csize = (int64_t)le32(h + 4);
        const int64_t body = pos + 8;
        if (std::memcmp(h, "fmt ", 4) == 0) {
            const int64_t avail = std::min<int64_t>(csize, form_end - body);
            if (avail < 16 || !fetch(body, 16, h)) { rc = AFSK_WAV_FORMAT; break; }
            const uint32_t tag = le16(h), channels = le16(h + 2), bits = le16(h + 14);
            const uint32_t width = (bits + 7) / 8;
            if (tag != 1 || channels == 0 || width == 0) { rc = AFSK_WAV_FORMAT; break; }
            framesize = (int64_t)channels * width;
        } else if (std::memcmp(h, "data", 4) == 0) {
            if (framesize == 0) { rc = AFSK_WAV_NO_DATA; break; }       // 'data' before 'fmt '
            const int64_t want = (csize / framesize) * framesize;      // getnframes() whole frames
            const int64_t avail = std::max<int64_t>(0, form_end - body);
            *data_off = body;
            *data_bytes = std::min(want, avail);
            rc = AFSK_WAV_OK;
            break;
        }
        pos = body + csize + (csize & 1);                               // chunks are padded to even sizes
    }
    return rc;
}

int wav_probe_one(const char* path, int64_t* data_off, int64_t* data_bytes) {
    *data_off = 0; *data_bytes = 0;
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return AFSK_WAV_IO;
    const int rc = wav_probe_fd(fd, data_off, data_bytes);
    close(fd);
    return rc;
}

// Interpret the canonical 44-byte header (what the stdlib writer behind SoundOutput.writeToFile produces,
// ref:256-263) of a file of `file_size` bytes: true and the bytes readframes(getnframes()) covers, which start at
// byte 44 -- or false: not this layout, or a file the chunk walk above has to judge.
bool wav_canonical_data(const unsigned char* hdr, int64_t file_size, int64_t* data_bytes) {
    if (std::memcmp(hdr, "RIFF", 4) != 0 || std::memcmp(hdr + 8, "WAVEfmt ", 8) != 0 || le32(hdr + 16) != 16 ||
        std::memcmp(hdr + 36, "data", 4) != 0)
        return false;
    const uint32_t tag = le16(hdr + 20), channels = le16(hdr + 22), width = (le16(hdr + 34) + 7) / 8;
    const int64_t framesize = (int64_t)channels * width;
    const int64_t csize = (int64_t)le32(hdr + 40);
    // (a RIFF size field below 36 puts a chunk header outside the form: the stdlib reader -- and
    // wav_probe_fd, which demands pos + 8 <= form_end for both chunk headers -- rejects such a file,
    // so it must not be reported OK with 0 data bytes here: the general walk gives its status)
    const int64_t form_end = std::min<int64_t>(file_size, 8 + (int64_t)le32(hdr + 4));
    if (tag != 1 || framesize <= 0 || form_end < 44) return false;
    const int64_t want = (csize / framesize) * framesize;          // getnframes() whole frames
    const int64_t avail = std::max<int64_t>(0, form_end - 44);
    *data_bytes = std::min(want, avail);
    return true;
}

// what wave.Wave_write emits for 1 ch / 16 bit / 48000 Hz
void wav_canonical_header(unsigned char* h, uint32_t data_bytes) {
    std::memcpy(h, "RIFF", 4); put_le32(h + 4, 36u + data_bytes); std::memcpy(h + 8, "WAVEfmt ", 8); put_le32(h + 16, 16u);
    put_le16(h + 20, 1u); put_le16(h + 22, 1u); put_le32(h + 24, AFSK_SAMPLE_RATE); put_le32(h + 28, AFSK_SAMPLE_RATE * 2u); put_le16(h + 32, 2u);
    put_le16(h + 34, 16u); std::memcpy(h + 36, "data", 4); put_le32(h + 40, data_bytes);
}

}  // namespace
