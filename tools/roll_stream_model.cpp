// CPU replay of the slice stream and ring protocol of the rolling conv kernels (dffw_conv_roll.hip, dffw_conv_rollx.hip), driven by the SAME
// schedule functions the kernels use (roll_sched / roll_step, dffw_conv_roll.h).  No GPU, no HIP runtime call: a host program, built with
// -fsanitize=address,undefined by tests/test_roll_stream_model.py.
//
// A workgroup is replayed the way the kernels are written: a fill cursor that walks the units' stream entries (RING - 1 entries in the prologue,
// then exactly one per step, past the end of the stream too) and a step cursor that walks the units' steps; entry f goes to ring slot f % RING.
// For every body's (RING, slices that may stay in flight across a step's barrier) and every B, N, zsplit and units-per-workgroup of the sweep:
//   * every output slice of every unit is produced exactly once;
//   * step n reads ring slots n, n+1, n+2, and every slot a live, present tap reads holds that unit's slice centre-1 / centre / centre+1;
//   * that slice had landed at the barrier in front of the step: queued early enough for the counted wait to cover it;
//   * the fill issued inside a step never targets a slot the step reads (a slot is refilled behind the barrier after its last reader);
//   * a unit over the whole slice range takes exactly nz steps, all live.
// usage: roll_stream_model            (exit code 0 and one summary line, or the first violation and exit code 1)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dffw_conv_roll.h"

using dffw::roll_sched;
using dffw::roll_step;
using dffw::RollSched;

struct Body {
    const char *name;
    int ring;       // ring slots; the fill cursor runs ring - 1 entries ahead of the window
    int inflight;   // slices whose DMA may still be in flight across a step's barrier (the counted vmcnt)
};
// conv_roll / conv_roll_t: INFLIGHT = (RING - 4) * PPW, with a prefetched residual PPW; conv_roll_t32: ring 4 (row phase 0) or 6; conv_roll_efd: ring 5;
// conv_roll_s2: rings 5 / 6 / 4; conv_rollx_pair: ring 6, two slices; conv_rollx_k2: ring 5, one
static const Body kBodies[] = {
    {"conv_roll", 6, 2},      {"conv_roll+res", 6, 1},     {"conv_roll_t", 6, 2},       {"conv_roll_t+res", 6, 1},  {"conv_roll_t32<0>", 4, 0},
    {"conv_roll_t32<1>", 6, 2}, {"conv_roll_t32<1>+res", 6, 1}, {"conv_roll_efd", 5, 1},    {"conv_roll_s2<kh2>", 5, 1}, {"conv_roll_s2<nt2>", 6, 2},
    {"conv_roll_s2<nt1>", 4, 0}, {"conv_rollx_pair", 6, 2},   {"conv_rollx_k2", 5, 1},
};

// ---- the chunk lists (RollChunks): the chunks of an absent slice leave, the others keep their K order ----
template <class CH, int... C>
constexpr bool chunks_are() {
    constexpr int want[] = {C...};
    if (CH::N != (int)sizeof...(C)) return false;
    for (int i = 0; i < CH::N; ++i)
        if (CH::at(i) != want[i]) return false;
    return true;
}
using dffw::ROLL_NO_BACK;
using dffw::ROLL_NO_FRONT;
using dffw::RollChunks;
static_assert(RollChunks<dffw::DzRoll, 15, 0>::N == 15 && RollChunks<dffw::DzRoll, 15, 0>::at(7) == 7, "full list");
static_assert(chunks_are<RollChunks<dffw::DzRoll, 15, ROLL_NO_FRONT>, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14>(), "plain form without its front slice");
static_assert(chunks_are<RollChunks<dffw::DzRoll, 15, ROLL_NO_BACK>, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9>(), "plain form without its back slice");
static_assert(chunks_are<RollChunks<dffw::DzRoll, 15, ROLL_NO_FRONT | ROLL_NO_BACK>, 5, 6, 7, 8, 9>(), "plain form, one slice");
static_assert(chunks_are<RollChunks<dffw::DzPair, 18, ROLL_NO_FRONT | ROLL_NO_BACK>, 6, 7, 8, 9, 10, 11>(), "pair form, one slice");
static_assert(chunks_are<RollChunks<dffw::DzT, 9, ROLL_NO_FRONT>, 1, 2, 5, 6, 7, 8>(), "transposed: both row phases lose their front chunks");
static_assert(chunks_are<RollChunks<dffw::DzT, 9, ROLL_NO_BACK>, 0, 1, 3, 4, 5, 6>(), "transposed without its back slice");
static_assert(chunks_are<RollChunks<dffw::DzT, 9, ROLL_NO_FRONT | ROLL_NO_BACK>, 1, 5, 6>(), "transposed, one slice");
static_assert(chunks_are<RollChunks<dffw::DzT32<1>, 9, ROLL_NO_FRONT>, 1, 2, 5, 6, 7, 8>(), "transposed 32, row phase 0");
static_assert(chunks_are<RollChunks<dffw::DzT32<2>, 18, ROLL_NO_BACK>, 0, 1, 2, 3, 6, 7, 8, 9, 10, 11, 12, 13>(), "transposed 32, row phase 1");
static_assert(chunks_are<RollChunks<dffw::DzEfd, 18, ROLL_NO_FRONT>, 3, 4, 5, 6, 7, 8, 12, 13, 14, 15, 16, 17>(), "EFD block: both branches");
static_assert(chunks_are<RollChunks<dffw::DzEfd, 9, ROLL_NO_FRONT | ROLL_NO_BACK>, 3, 4, 5>(), "strided conv, one slice");

struct Unit {
    int b, col, zbeg, nz;
};
struct Entry {
    int unit;   // index into the workgroup's unit list; -1: past the end of the stream
    int z;      // input slice; outside [0, ni): zero page / dummy
};

static int g_checks = 0;
#define REQUIRE(cond, ...)                \
    do {                                  \
        ++g_checks;                       \
        if (!(cond)) {                    \
            fprintf(stderr, "FAIL: ");    \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            exit(1);                      \
        }                                 \
    } while (0)

// units are numbered column fastest, then slice range, then sample (roll_unit, dffw_persist.h)
static Unit decode(int u, int cols, int zsplit, int no) {
    Unit c;
    c.col = u % cols;
    int tt = u / cols;
    const int zp = tt % zsplit;
    c.b = tt / zsplit;
    c.zbeg = zp * no / zsplit;
    c.nz = (zp + 1) * no / zsplit - c.zbeg;
    return c;
}

static void replay(const Body &body, int B, int N, int zsplit, int cols, int ufirst, int ustep, std::vector<int> &produced) {
    const int total = B * zsplit * cols, RING = body.ring;
    std::vector<Unit> units;
    for (int u = ufirst; u < total; u += ustep) units.push_back(decode(u, cols, zsplit, N));
    if (units.empty()) return;
    const int nu = (int)units.size();

    // ---- the fill cursor, as in the kernels: setup_fill() per unit, issue_next() per ring fill
    std::vector<Entry> slot(RING, Entry{-2, 0});
    std::vector<Entry> queued;   // every fill in issue order
    int fu = 0, fq = 0, fslot = 0;
    RollSched fs = roll_sched(units[0].zbeg, units[0].nz, N, true);
    auto issue_next = [&]() {
        Entry e{fu < nu ? fu : -1, fu < nu ? fs.z0 + fq : -1};
        slot[fslot] = e;
        queued.push_back(e);
        fslot = (fslot + 1 == RING) ? 0 : fslot + 1;
        if (fu < nu && ++fq == fs.fills) {
            fq = 0;
            ++fu;
            if (fu < nu) fs = roll_sched(units[fu].zbeg, units[fu].nz, N, false);
        }
    };
    for (int q = 0; q < RING - 1; ++q) issue_next();

    // ---- the step cursor
    int n = 0, sidx = 0;   // step number of the workgroup; ring slot of the window's first slice
    for (int cu = 0; cu < nu; ++cu) {
        const Unit &U = units[cu];
        const RollSched sc = roll_sched(U.zbeg, U.nz, N, cu == 0);
        if (zsplit == 1) REQUIRE(sc.steps == U.nz, "%s: full-range unit takes %d steps for %d slices", body.name, sc.steps, U.nz);
        for (int st = 0; st < sc.steps; ++st, ++n) {
            const int mode = roll_step(sc, st, U.zbeg, U.nz, N);
            if (zsplit == 1) REQUIRE(mode & dffw::ROLL_LIVE, "%s: dead step in a full-range unit", body.name);
            const int fill_target = fslot;
            issue_next();   // exactly one fill per step, in front of the contraction
            REQUIRE((int)queued.size() == n + RING, "%s: fill count", body.name);
            REQUIRE(sidx == n % RING, "%s: window slot", body.name);
            if (mode & dffw::ROLL_LIVE) {
                const int centre = sc.c0 + st;
                ++produced[(U.b * N + centre) * cols + U.col];
                for (int dz = 0; dz < 3; ++dz) {
                    if ((dz == 0 && (mode & dffw::ROLL_NO_FRONT)) || (dz == 2 && (mode & dffw::ROLL_NO_BACK))) continue;
                    const int sl = (sidx + dz) % RING, want = centre - 1 + dz;
                    REQUIRE(want >= 0 && want < N, "%s: a present tap outside the volume (slice %d of %d)", body.name, want, N);
                    REQUIRE(sl != fill_target, "%s: step %d reads slot %d while it is being refilled", body.name, n, sl);
                    REQUIRE(slot[sl].unit == cu && slot[sl].z == want, "%s: B %d N %d zsplit %d step %d tap %d: slot %d holds (unit %d, slice %d), wanted (unit %d, slice %d)",
                            body.name, B, N, zsplit, n, dz, sl, slot[sl].unit, slot[sl].z, cu, want);
                    // stream entry n + dz; at the barrier in front of step n (the one that ended step n - 1, or the prologue's full wait) entries up to
                    // (n - 1) + RING - 1 - inflight have landed
                    REQUIRE(queued[n + dz].unit == cu && queued[n + dz].z == want, "%s: step %d tap %d is not stream entry %d", body.name, n, dz, n + dz);
                    REQUIRE(n == 0 || n + dz <= n - 1 + RING - 1 - body.inflight, "%s: step %d tap %d read before its slice has landed", body.name, n, dz);
                }
            }
            sidx = (sidx + 1 == RING) ? 0 : sidx + 1;
        }
    }
    REQUIRE(fu >= nu, "%s: the fill cursor did not reach the end of the stream", body.name);
}

int main() {
    const int Bs[] = {1, 2, 3}, Ns[] = {1, 2, 3, 4, 10}, Zs[] = {1, 2, 3};
    const int cols = 3;
    int runs = 0;
    for (const Body &body : kBodies)
        for (int B : Bs)
            for (int N : Ns)
                for (int zsplit : Zs) {
                    if (zsplit > N) continue;   // the host never splits a sample into more ranges than it has slices
                    const int total = B * zsplit * cols;
                    // one "XCD": `ustep` workgroups take the units round-robin, from all units in one workgroup (ustep 1) to one unit each (ustep total)
                    for (int ustep = 1; ustep <= total; ++ustep) {
                        std::vector<int> produced(B * N * cols, 0);
                        for (int ufirst = 0; ufirst < ustep; ++ufirst) replay(body, B, N, zsplit, cols, ufirst, ustep, produced);
                        for (int v : produced) REQUIRE(v == 1, "%s: B %d N %d zsplit %d: an output slice produced %d times", body.name, B, N, zsplit, v);
                        ++runs;
                    }
                }
    printf("roll_stream_model: %d launches replayed, %d checks, all passed\n", runs, g_checks);
    return 0;
}
