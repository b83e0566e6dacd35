/*
 * survivor_check — the self-delimiting survivor lists of the marking (disco_amd/csrc/disco_survivor.h) exercised on the host: the
 * same header the kernels include, built as plain C++. Every length 0..4 and wide round trips, the sentinel of a node without a
 * survivor is no entry, and whatever an earlier pass left behind the mark is never read.
 *   survivor_check            -> "ok N checks", exit 0; the first failed check is printed and the exit status is 1
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../csrc/disco_survivor.h"

typedef unsigned long long u64;

static unsigned long checks = 0;
#define CHECK(x)                                                          \
    do {                                                                  \
        ++checks;                                                         \
        if (!(x)) {                                                       \
            fprintf(stderr, "line %d: %s\n", __LINE__, #x);               \
            return 1;                                                     \
        }                                                                 \
    } while (0)

/* an adjacency entry as disco_device.h packs it: offset(15) | dst(31) | orient(2) | bit 15 clear | len(dst)(15) */
static u64 entry(u64 off, u64 dst, u64 o, u64 dlen) { return (off << 49) | (dst << 18) | (o << 16) | dlen; }

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd()
{
    rng_state ^= rng_state << 7;
    rng_state ^= rng_state >> 9;
    return rng_state * 0x2545F4914F6CDD1Dull;
}
static u64 random_entry() { return entry(rnd() % 0x8000, rnd() % 0x80000000ull, rnd() & 3, 1 + rnd() % 0x7FFF); } /* (a read has a length) */

int main()
{
    static_assert(SURV_CAP == 4, "four slots");
    CHECK((SURV_NONE & 0x7FFFull) == 0 && surv_entry(SURV_NONE) == 0); /* the sentinel: the mark alone, no entry */
    for (int round = 0; round < 20000; round++) {
        u64 e[8];
        for (u64 &x : e) x = random_entry();
        for (unsigned i = 0; i < 8; i++) CHECK(!(e[i] & SURV_LAST));
        const u64 other = random_entry();
        for (unsigned n = 0; n <= 8; n++) { /* survivors of the node; more than four: wide */
            /* the slots as an earlier pass left them: entries with and without marks, sentinels, zeroes, all ones */
            u64 slot[SURV_CAP];
            for (unsigned r = 0; r < SURV_CAP; r++) {
                switch (rnd() % 5) {
                case 0: slot[r] = random_entry(); break;
                case 1: slot[r] = random_entry() | SURV_LAST; break;
                case 2: slot[r] = SURV_NONE; break;
                case 3: slot[r] = 0; break;
                default: slot[r] = ~0ull; break;
                }
            }
            /* what the marking stores: the first four survivors, the last one marked; none: the sentinel in slot 0 */
            for (unsigned r = 0; r < n && r < SURV_CAP; r++) slot[r] = surv_encode(e[r], r, n);
            if (n == 0) slot[0] = SURV_NONE;
            const unsigned len = surv_len(slot[0], slot[1], slot[2], slot[3]);
            CHECK(len == (n <= SURV_CAP ? n : (unsigned)SURV_WIDE));
            for (unsigned r = 0; r < n && r < SURV_CAP; r++) CHECK(surv_entry(slot[r]) == e[r]);
            for (unsigned r = 0; r < 8; r++) { /* membership: the survivors, and nothing that sits behind the mark */
                const bool in_list = n <= SURV_CAP && r < n;
                bool same_as_member = false; /* (random entries may repeat) */
                for (unsigned q = 0; q < n && q < SURV_CAP; q++) same_as_member |= (e[q] == e[r]);
                if (in_list) CHECK(surv_has(slot[0], slot[1], slot[2], slot[3], e[r]));
                else if (n <= SURV_CAP && !same_as_member) CHECK(!surv_has(slot[0], slot[1], slot[2], slot[3], e[r]));
                if (n > SURV_CAP) CHECK(!surv_has(slot[0], slot[1], slot[2], slot[3], e[r])); /* wide: the row is asked */
            }
            if (n <= SURV_CAP) {
                bool member = false;
                for (unsigned q = 0; q < n; q++) member |= (e[q] == other);
                CHECK(surv_has(slot[0], slot[1], slot[2], slot[3], other) == member);
                /* stale garbage behind the mark is not matched even when it IS the value asked for */
                for (unsigned r = n ? n : 1; r < SURV_CAP; r++) {
                    u64 s2[SURV_CAP] = {slot[0], slot[1], slot[2], slot[3]};
                    s2[r] = other;
                    CHECK(surv_has(s2[0], s2[1], s2[2], s2[3], other) == member);
                    s2[r] = other | SURV_LAST;
                    CHECK(surv_has(s2[0], s2[1], s2[2], s2[3], other) == member);
                    CHECK(surv_len(s2[0], s2[1], s2[2], s2[3]) == n);
                }
            }
        }
    }
    printf("ok %lu checks\n", checks);
    return 0;
}
