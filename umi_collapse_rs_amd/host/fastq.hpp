// FASTQ input of `umicollapse -m fastq`: the whole file, plain or gzip (any number of members, BGZF
// included), and its four-line records.  The reference's fastq mode is a TODO (src/main.rs:49-50);
// what a record is and which inputs are refused is this build's definition (umicollapse_main.cpp).
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include <zlib.h>

#include "bgzf.hpp"

namespace umi {
namespace fastq {

// The file's bytes, inflated when it starts with the gzip magic (1f 8b).  A plain zlib stream reader
// rather than the BGZF Inflater: gzip as written by gzip(1) has no block sizes to split on.  Members
// follow each other until the input ends (concatenated gzip, BGZF's blocks, its empty EOF block).
inline bgzf::Bytes read_all(const std::string &path, unsigned threads)
{
    bgzf::Bytes raw = bgzf::read_file(path, threads);
    if (raw.size() < 2 || raw[0] != 0x1f || raw[1] != 0x8b) return raw;
    bgzf::Bytes out;
    out.resize(std::max<size_t>(raw.size() * 4, 1u << 16));
    z_stream zs{};
    if (inflateInit2(&zs, 15 + 16) != Z_OK) throw bgzf::IoError("inflateInit2 failed");
    size_t in_off = 0, out_off = 0;
    for (;;) {
        zs.next_in = raw.data() + in_off;
        zs.avail_in = (uInt)std::min<size_t>(raw.size() - in_off, 1u << 30);
        if (out.size() - out_off < (1u << 16)) out.resize(out.size() * 2);
        zs.next_out = out.data() + out_off;
        zs.avail_out = (uInt)std::min<size_t>(out.size() - out_off, 1u << 30);
        const uInt in0 = zs.avail_in, out0 = zs.avail_out;
        const int rc = inflate(&zs, Z_NO_FLUSH);
        in_off += in0 - zs.avail_in;
        out_off += out0 - zs.avail_out;
        if (rc == Z_STREAM_END) {
            if (in_off >= raw.size()) break;
            inflateReset(&zs); // the next member
            continue;
        }
        if (rc == Z_BUF_ERROR && in0 == zs.avail_in && out0 == zs.avail_out) {
            inflateEnd(&zs);
            throw bgzf::IoError("truncated gzip stream in " + path);
        }
        if (rc != Z_OK && rc != Z_BUF_ERROR) {
            inflateEnd(&zs);
            throw bgzf::IoError("corrupt gzip stream in " + path + (zs.msg ? std::string(": ") + zs.msg : ""));
        }
    }
    inflateEnd(&zs);
    out.resize(out_off);
    return out;
}

// One record: the four lines as offsets into the file's bytes (without their '\n').
struct Record {
    size_t head, head_len; // "@..." line
    size_t seq, len;       // sequence (len bases)
    size_t plus, plus_len; // "+..." line
    size_t qual;           // quality (len characters)
};

// Splits the text into records; returns "" or the first problem (record number 1-based).
inline std::string parse(const uint8_t *d, size_t n, std::vector<Record> &out)
{
    size_t p = 0;
    auto line = [&](size_t &start, size_t &len) -> bool {
        if (p >= n) return false;
        start = p;
        const void *nl = std::memchr(d + p, '\n', n - p);
        const size_t e = nl ? (size_t)((const uint8_t *)nl - d) : n;
        len = e - p;
        p = nl ? e + 1 : n;
        return true;
    };
    for (size_t rec = 1; p < n; rec++) {
        Record r;
        size_t qlen = 0;
        if (!line(r.head, r.head_len)) break;
        if (r.head_len == 0 || d[r.head] != '@')
            return "FASTQ record " + std::to_string(rec) + ": the header line does not start with '@'";
        if (!line(r.seq, r.len) || !line(r.plus, r.plus_len) || !line(r.qual, qlen))
            return "FASTQ record " + std::to_string(rec) + ": truncated record";
        if (r.plus_len == 0 || d[r.plus] != '+')
            return "FASTQ record " + std::to_string(rec) + ": the third line does not start with '+'";
        if (qlen != r.len)
            return "FASTQ record " + std::to_string(rec) + ": sequence and quality differ in length (" +
                   std::to_string(r.len) + " vs " + std::to_string(qlen) + ")";
        out.push_back(r);
    }
    return "";
}

// (int)(sum(q - 33) as f32 / len as f32): the SAM path's get_avg_qual (src/utils/read.rs:55-61) with
// Phred+33 taken off; integer partial sums below 2^24 are what the running f32 sum holds exactly
inline int32_t avg_qual(const uint8_t *q, size_t len)
{
    if (len == 0) return 0; // 0.0 / 0.0 is NaN, and NaN as i32 is 0
    int64_t s = 0;
    for (size_t i = 0; i < len; i++) s += (int64_t)q[i] - 33;
    return (int32_t)((float)s / (float)len);
}

} // namespace fastq
} // namespace umi
