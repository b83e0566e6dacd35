/* The host's end of the pinned ring that outputs leave through: a piece lies in one half of the ring and belongs at one or more
 * destinations — files at offsets, or the caller's memory. Plain C++ (no HIP, no context): disco_hip.hip delivers every piece with
 * this, and disco_amd/host/ringio_check.cpp holds it to a file's bytes on its own. */
#pragma once
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace ringio {

/* `len` bytes at `src` belong at byte `off` of the file `fd`, or — host != null — of the memory at `host` */
struct Segment {
    const char *src = nullptr;
    size_t len = 0;
    int fd = -1;
    char *host = nullptr;
    uint64_t off = 0;
};

/* pwrite until the bytes are in the file; false: the file takes no more (or nothing at all: a descriptor not open for writing) */
inline bool write_all(int fd, const char *src, size_t len, uint64_t off)
{
    size_t done = 0;
    while (done < len) {
        const ssize_t w = pwrite(fd, src + done, len - done, (off_t)(off + done));
        if (w <= 0) return false;
        done += (size_t)w;
    }
    return true;
}

/* the bytes [b, e) of a segment to where they belong */
inline bool put(const Segment &s, size_t b, size_t e)
{
    if (s.host) {
        if (e > b) memcpy(s.host + s.off + b, s.src + b, e - b); /* (an empty segment may have no address) */
        return true;
    }
    return write_all(s.fd, s.src + b, e - b, s.off + b);
}

/* how one segment is cut among writers: min(threads, 64) of them, none for less than 64 KB, slices of whole 4 KB pages */
inline void split_plan(size_t len, unsigned threads, size_t *writers, size_t *slice)
{
    const size_t cap = std::max<size_t>(1, std::min<unsigned>(threads, 64));
    *writers = std::max<size_t>(1, std::min<size_t>(cap, len >> 16));
    *slice = ((len + *writers - 1) / *writers + 4095) & ~(size_t)4095;
}

/* one segment split among writers at disjoint offsets: the bytes of ONE file, whose writes serialise on its inode lock when they
 * come from one thread after the other only */
inline bool deliver_split(const Segment &s, unsigned threads)
{
    size_t writers, slice;
    split_plan(s.len, threads, &writers, &slice);
    if (writers == 1) return put(s, 0, s.len);
    std::atomic<bool> ok{true};
    std::vector<std::thread> th;
    for (size_t b = 0; b < s.len; b += slice)
        th.emplace_back([&s, &ok, b, slice]() {
            if (!put(s, b, std::min(s.len, b + slice))) ok.store(false);
        });
    for (auto &x : th) x.join();
    return ok.load();
}

/* several segments, one writer each (a round of the text files: every file has its own inode lock); an empty segment has none */
inline bool deliver_each(const Segment *segs, size_t n)
{
    std::atomic<bool> ok{true};
    std::vector<std::thread> th;
    for (size_t i = 0; i < n; i++)
        if (segs[i].len)
            th.emplace_back([&ok, s = segs + i]() {
                if (!put(*s, 0, s->len)) ok.store(false);
            });
    for (auto &x : th) x.join();
    return ok.load();
}

} /* namespace ringio */
