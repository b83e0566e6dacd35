/*
 * ringio_check — the host's end of the output ring (disco_amd/csrc/disco_ringio.h) on its own: the header disco_hip.hip delivers every
 * piece with, built as plain C++. A segment split among writers lands at a non-zero offset of a file full of a sentinel byte and
 * changes nothing around it, at every size where the split changes (no writer for less than 64 KB, slices of whole 4 KB pages, at
 * most 64 writers); the same into memory; a piece of several segments with a writer each; a file that takes no bytes is reported.
 *   ringio_check DIR          -> "ok N checks", exit 0; the first failed check is printed and the exit status is 1
 */
#include <fcntl.h>

#include <cstdio>
#include <cstdlib>
#include <string>

#include "../csrc/disco_ringio.h"

static unsigned long checks = 0;
#define CHECK(x)                                            \
    do {                                                    \
        ++checks;                                           \
        if (!(x)) {                                         \
            fprintf(stderr, "line %d: %s\n", __LINE__, #x); \
            return 1;                                       \
        }                                                   \
    } while (0)

static const unsigned char SENTINEL = 0xA5;
static const size_t FRONT = 4099, BACK = 8193; /* the bytes around the range: the range begins at no page boundary */

/* bytes that differ from the sentinel and from each other at page distance */
static std::vector<char> pattern(size_t n, unsigned seed)
{
    std::vector<char> v(n);
    unsigned long long x = 0x9E3779B97F4A7C15ull + seed;
    for (size_t i = 0; i < n; i++) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        unsigned char b = (unsigned char)(x >> 56);
        v[i] = (char)(b == SENTINEL ? 0x5A : b);
    }
    return v;
}

static bool fill(int fd, size_t n)
{
    const std::vector<char> s(n, (char)SENTINEL);
    return ftruncate(fd, 0) == 0 && ringio::write_all(fd, s.data(), n, 0);
}

/* the file holds `src` at [at, at + n) and the sentinel everywhere else, and is size bytes long */
static bool holds(int fd, size_t size, size_t at, const char *src, size_t n)
{
    std::vector<char> got(size + 1);
    const ssize_t r = pread(fd, got.data(), size + 1, 0);
    if (r != (ssize_t)size) return false;
    for (size_t i = 0; i < size; i++) {
        const char want = i >= at && i < at + n ? src[i - at] : (char)SENTINEL;
        if (got[i] != want) return false;
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: ringio_check DIR\n");
        return 2;
    }
    const std::string path = std::string(argv[1]) + "/ringio_check.bin";
    const int fd = open(path.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0600);
    CHECK(fd >= 0);
    const size_t sizes[] = {0, 1, 65535, 65536, 65537, 3 * 4096 + 1, 5u * 1024 * 1024 + 3};
    const unsigned threads[] = {1, 2, 16, 64, 100};
    unsigned seed = 0;
    for (size_t n : sizes)
        for (unsigned t : threads) {
            /* the plan: what the writers of the records and of the GFA text have always done */
            size_t writers, slice;
            ringio::split_plan(n, t, &writers, &slice);
            CHECK(writers >= 1 && writers <= 64 && writers <= std::max(1u, t));
            CHECK(writers == 1 || n / writers >= 65536); /* no extra writer for less than 64 KB each */
            CHECK(slice % 4096 == 0 && slice * writers >= n);
            const std::vector<char> src = pattern(n, seed++);
            ringio::Segment s;
            s.src = src.data();
            s.len = n;
            /* into the file, at an offset */
            const size_t size = FRONT + n + BACK;
            CHECK(fill(fd, size));
            s.fd = fd;
            s.off = FRONT;
            CHECK(ringio::deliver_split(s, t));
            CHECK(holds(fd, size, FRONT, src.data(), n));
            /* into memory */
            std::vector<char> mem(size, (char)SENTINEL);
            s.fd = -1;
            s.host = mem.data();
            CHECK(ringio::deliver_split(s, t));
            for (size_t i = 0; i < size; i++) CHECK(mem[i] == (i >= FRONT && i < FRONT + n ? src[i - FRONT] : (char)SENTINEL));
        }
    /* a piece of several segments, a writer each: three files and a stretch of memory, two of the segments empty */
    {
        const size_t lens[5] = {70000, 0, 4096, 0, 12345};
        const std::vector<char> half = pattern(5 * 131072, seed++); /* the segments lie 128 KB apart in the half */
        int fds[4];
        std::vector<char> mem(FRONT + lens[4] + BACK, (char)SENTINEL);
        ringio::Segment segs[5];
        for (int i = 0; i < 5; i++) {
            segs[i].src = half.data() + (size_t)i * 131072;
            segs[i].len = lens[i];
            segs[i].off = FRONT + (size_t)i;
            if (i < 4) {
                const std::string p = path + "." + std::to_string(i);
                fds[i] = open(p.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0600);
                CHECK(fds[i] >= 0);
                CHECK(fill(fds[i], FRONT + i + lens[i] + BACK));
                segs[i].fd = fds[i];
                unlink(p.c_str());
            } else
                segs[i].host = mem.data();
        }
        CHECK(ringio::deliver_each(segs, 5));
        for (int i = 0; i < 4; i++) {
            CHECK(holds(fds[i], FRONT + i + lens[i] + BACK, FRONT + i, segs[i].src, lens[i]));
            close(fds[i]);
        }
        for (size_t i = 0; i < mem.size(); i++) CHECK(mem[i] == (i >= FRONT + 4 && i < FRONT + 4 + lens[4] ? segs[4].src[i - FRONT - 4] : (char)SENTINEL));
        CHECK(ringio::deliver_each(segs, 0)); /* no segment at all */
    }
    /* a file that takes no bytes: reported by every way in, and the file is as it was */
    {
        const std::vector<char> src = pattern(300000, seed++);
        CHECK(fill(fd, FRONT + src.size() + BACK));
        const int ro = open(path.c_str(), O_RDONLY);
        CHECK(ro >= 0);
        CHECK(!ringio::write_all(ro, src.data(), 1, 0));
        ringio::Segment s;
        s.src = src.data();
        s.len = src.size();
        s.fd = ro;
        s.off = FRONT;
        CHECK(!ringio::deliver_split(s, 1));
        CHECK(!ringio::deliver_split(s, 4));
        ringio::Segment two[2] = {s, s};
        two[1].fd = fd; /* (one of two fails: the piece has failed; the other segment is written) */
        CHECK(!ringio::deliver_each(two, 2));
        CHECK(holds(fd, FRONT + src.size() + BACK, FRONT, src.data(), src.size()));
        close(ro);
    }
    close(fd);
    unlink(path.c_str());
    printf("ok %lu checks\n", checks);
    return 0;
}
