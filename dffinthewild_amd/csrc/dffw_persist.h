// The persistent-grid contract of the streaming kernels, and the instantiation table their launchers read.
//
// A streaming launch covers `total_tiles` units (columns of a sample, or slice ranges of them) with a grid that is a multiple of the 8 XCDs.
// Workgroup b runs on XCD b % 8; XCD x owns a CONTIGUOUS range of the units (the first total % 8 XCDs one unit more than the rest) and its
// gridDim.x / 8 workgroups take that range round-robin, so the workgroups that run at the same time on an XCD walk neighbouring columns and share
// their halos in that XCD's L2.  persistent_grid() (host) and persistent_range() (device) are the two halves of that rule: nothing else computes either.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "dffw_conv_roll.h"

namespace dffw {

// `want` workgroups (the launcher's default or RollArgs/SrdArgs::wgs), rounded down to a multiple of 8, never more per XCD than it has units
inline unsigned persistent_grid(int total_tiles, int want) {
    const int per_xcd = (total_tiles + 7) / 8;
    return (unsigned)(8 * std::min(per_xcd, std::max(1, want / 8)));
}

// One instantiation of a kernel family: what a launch reports (last_conv_kernel(), the dispatch pins, rocprofv3 matching), the kernel and its block
// size.  DFFW_ROW spells the name from the template arguments it instantiates, defaulted ones included, so the name IS the kernel symbol; a row
// written out by hand carries a label that is not (kept where the pinned spelling is a shortened one).  A new instantiation is one new row.
template <class... A>
struct KernelRow {
    const char *name;
    void (*fn)(A...);
    int block;
};
#define DFFW_ROW_(block, kernel, ...) {"dffw::" #kernel "<" #__VA_ARGS__ ">", kernel<__VA_ARGS__>, block}
#define DFFW_ROW(block, kernel, ...) DFFW_ROW_(block, kernel, __VA_ARGS__)

// the tables are written with the precisions as numerals (they are spelled into the names) and indexed by them
static_assert(P_BF16X3 == 0 && P_FP16 == 1 && P_BF16 == 2, "the launch tables index rows by precision");

// a table laid out [precision][per_prec variants]: the row of (prec, sub), null for a precision that does not exist
template <class Row>
inline const Row *prec_row(const Row *table, int prec, int per_prec, int sub) {
    return prec == P_BF16X3 || prec == P_FP16 || prec == P_BF16 ? &table[prec * per_prec + sub] : nullptr;
}

#ifdef DFFW_ABL_BUILD
// development (make ABL=1): an extra instantiation and the value of the environment switch that selects it, in one place
template <class Row>
struct AblRow {
    int value;
    Row row;
};
template <class Row, int N>
inline const Row *abl_row(const AblRow<Row> (&table)[N], const char *env) {
    const char *z = getenv(env);
    for (int i = 0; z && i < N; ++i)
        if (atoi(z) == table[i].value) return &table[i].row;
    return nullptr;
}
#endif

using RollRow = KernelRow<ConvArgs, RollArgs>;   // the conv_roll* / conv_slice* / conv_efd16 families

template <class... A>
inline void copy_row_name(const KernelRow<A...> *row, char *buf, int n) {
    if (n > 0) snprintf(buf, n, "%s", row ? row->name : "");
}

// select()'s row on the persistent grid; a null row (no instantiation for these arguments) is an invalid launch
template <class... A, class... B>
inline hipError_t launch_row(const KernelRow<A...> *row, int total_tiles, int want, unsigned grid_y, hipStream_t s, const B &...args) {
    if (!row) return hipErrorInvalidValue;
    hipLaunchKernelGGL(row->fn, dim3(persistent_grid(total_tiles, want), grid_y), dim3(row->block), 0, s, args...);
    return hipGetLastError();
}

// a reducing family's launch: `row` on `grid`, then its finish kernel on `fgrid` blocks of 256 threads; the first error of the two
template <class Args, class... F, class... B>
inline hipError_t launch_row_then(const KernelRow<Args> *row, dim3 grid, const Args &a, hipStream_t s, void (*finish)(F...), unsigned fgrid, const B &...fargs) {
    if (!row) return hipErrorInvalidValue;
    hipLaunchKernelGGL(row->fn, grid, dim3(row->block), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(finish, dim3(fgrid), dim3(256), 0, s, fargs...);
    return hipGetLastError();
}

struct UnitRange {
    int first, end, step;   // this workgroup's units: first, first + step, ... below end (first >= end: nothing to do)
};
__device__ __forceinline__ UnitRange persistent_range(int total_tiles) {
    const int xcd = blockIdx.x & 7, widx = blockIdx.x >> 3, wgs_per_xcd = gridDim.x >> 3;
    const int q = total_tiles >> 3, rem = total_tiles & 7;
    const int xs = xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q;
    UnitRange r;
    r.end = xs + q + (xcd < rem ? 1 : 0);
    r.first = xs + widx;
    r.step = wgs_per_xcd;
    return r;
}

// unit u of a RollArgs launch: units are numbered x fastest, then y, slice range (zsplit), sample; a unit is a TY x TX column over output
// slices [zbeg, zbeg + nz) of sample b (`no` = the launch's output slices)
struct RollUnit {
    int b, zbeg, nz, gy0, gx0;
};
template <int TY, int TX>
__device__ __forceinline__ RollUnit roll_unit(int u, const RollArgs &t, int no) {
    RollUnit c;
    const int txi = u % t.tiles_x;
    int tt = u / t.tiles_x;
    const int tyi = tt % t.tiles_y;
    tt /= t.tiles_y;
    const int zp = tt % t.zsplit;
    c.b = tt / t.zsplit;
    c.gy0 = tyi * TY;
    c.gx0 = txi * TX;
    c.zbeg = zp * no / t.zsplit;
    c.nz = (zp + 1) * no / t.zsplit - c.zbeg;
    return c;
}

// f(M) for the step's absent-slice bits M as a compile-time constant: the step's chunk list is straight-line code behind one wave-uniform branch
template <class F>
__device__ __forceinline__ void roll_mode_switch(int mode, F &&f) {
    switch (mode & (ROLL_NO_FRONT | ROLL_NO_BACK)) {
        case 0: f(std::integral_constant<int, 0>{}); break;
        case ROLL_NO_FRONT: f(std::integral_constant<int, ROLL_NO_FRONT>{}); break;
        case ROLL_NO_BACK: f(std::integral_constant<int, ROLL_NO_BACK>{}); break;
        default: f(std::integral_constant<int, ROLL_NO_FRONT | ROLL_NO_BACK>{}); break;   // a volume of one slice
    }
}

}  // namespace dffw
