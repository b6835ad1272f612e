// Weight packing (dffw_pack.h): BatchNorm folding and the MFMA-fragment operand layouts of the conv kernels.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/dffw.h"
#include "dffw_conv_roll.h"
#include "dffw_align.h"
#include "dffw_srd_roll.h"
#include "dffw_pack.h"
#include "dffw_repack.h"

namespace dffw {

// ---- host number formats -----------------------------------------------------------------------
static uint16_t host_f2bf(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static float host_bf2f(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint16_t host_f2h(float f) {
    _Float16 h = (_Float16)f;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
static void host_split(int prec, float v, uint16_t &hi, uint16_t &lo) {
    if (prec == P_BF16X3) {
        hi = host_f2bf(v);
        lo = host_f2bf(v - host_bf2f(hi));
    } else if (prec == P_FP16) {
        hi = host_f2h(v);
        lo = 0;
    } else {
        hi = host_f2bf(v);
        lo = 0;
    }
}

// ---- plan mode (dffw_repack.h) -----------------------------------------------------
// plan_conv runs pack_conv once more with probe weights whose bit pattern is the source index + 1 and with BatchNorm ignored: what a fragment
// lambda returns is then the source of the slot (0.f: none).  While t_plan is set nothing is allocated or uploaded: upload() records the size of
// each buffer, in `owned` order, with the source map the writer left in t_next (none: a buffer without weights in it).
static thread_local LayerPlan *t_plan = nullptr;
static thread_local BufPlan t_next;
static int32_t src_of(float probe) {
    uint32_t u;
    memcpy(&u, &probe, 4);
    return (int32_t)u - 1;
}
static void plan_f32(std::vector<int32_t> &&map) {
    t_next.kind = RK_F32;
    t_next.map = std::move(map);
}

// ---- device buffers ----------------------------------------------------------------------------
void free_packed(PackedConv &pc) {
    for (void *p : pc.owned) (void)hipFree(p);
    pc = PackedConv();
}

// Copies `v` into a new device buffer that `pc` owns and points `dst` at it.  Each field is filled once: a second block packing
// the same field would mean two kernels claim one layer (and would lose the first buffer).
template <class T>
static int upload(PackedConv &pc, T *&dst, const std::vector<T> &v) {
    if (dst) return dffw_fail(DFFW_EINVAL, "pack_conv: layer %s packs one device buffer twice", pc.def.conv.c_str());
    if (t_plan) {
        t_next.bytes = v.size() * sizeof(T);
        t_plan->bufs.push_back(std::move(t_next));
        t_next = BufPlan();
        dst = reinterpret_cast<T *>(uintptr_t(64));   // never dereferenced: marks the field as packed for the check above
        return DFFW_OK;
    }
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, v.size() * sizeof(T));
    if (e == hipSuccess) {
        pc.owned.push_back(p);
        pc.owned_bytes.push_back(v.size() * sizeof(T));
        e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) return dffw_fail(DFFW_EHIP, "pack_conv: upload of %zu bytes -> %s", v.size() * sizeof(T), hipGetErrorString(e));
    dst = (T *)p;
    return DFFW_OK;
}

// The layout every MFMA operand buffer here shares: [fragment][part][64 lanes][8], part 1 = the low half of split-bf16 (only
// when prec_parts(prec) == 2).  w(f, lane, j) is the filter value element j of lane `lane` of fragment f carries (0: no weight).
template <class W>
static int pack_frags(PackedConv &pc, uint16_t *&dst, int prec, int nfrag, W &&w) {
    const int parts = prec_parts(prec);
    std::vector<uint16_t> buf((size_t)nfrag * parts * 512, 0);
    if (t_plan) {
        t_next.kind = RK_FRAGS;
        t_next.map.resize((size_t)nfrag * 512);
        for (int f = 0; f < nfrag; ++f)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) t_next.map[(size_t)f * 512 + (size_t)lane * 8 + j] = src_of(w(f, lane, j));
        return upload(pc, dst, buf);
    }
    for (int f = 0; f < nfrag; ++f)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
                uint16_t hi, lo;
                host_split(prec, w(f, lane, j), hi, lo);
                const size_t base = (size_t)f * parts * 512 + (size_t)lane * 8 + j;
                buf[base] = hi;
                if (parts == 2) buf[base + 512] = lo;
            }
    return upload(pc, dst, buf);
}

// filter tap t = 3 ky + kx of a 1x3x3 filter with pad (0, 1, 1)
static Tap tap_1x3x3(int t) { return Tap{0, t / 3 - 1, t % 3 - 1, 0, t / 3, t % 3}; }
// in-slice tap t = 3 ky + kx of filter slice kz of a 3x3x3 stride-1 filter with pad 1
static Tap tap_3x3x3(int kz, int t) { return Tap{kz - 1, t / 3 - 1, t % 3 - 1, kz, t / 3, t % 3}; }

int pack_conv(const LayerDef &L, int prec, const float *weight, const float *bn, const float *conv_bias,
              PackedConv &pc, const float *shortcut_w, int shortcut_cin) {
    pc.def = L;
    pc.nt = conv_nt_for(L.cout);
    const int parts = prec_parts(prec);
    const int cin_own = (L.cin + 7) / 8 * 8;
    const int cin_pad = cin_own + (shortcut_w ? (shortcut_cin + 7) / 8 * 8 : 0);   // channels of the (virtual) input concat
    const int c8n = cin_pad / 8;
    pc.cin_all = cin_pad;
    int rc = DFFW_OK;
    const bool plan = t_plan != nullptr;   // plan mode: `weight` / `shortcut_w` are probes, `bn` / `conv_bias` only say whether the layer has them
    const int64_t n_w = (int64_t)L.cin * L.cout * L.kd * L.kh * L.kw, n_sc = shortcut_w ? (int64_t)L.cout * shortcut_cin : 0;
    const int32_t shift_at = (int32_t)(n_w + n_sc), cbias_at = shift_at + L.cout;   // where the repack scratch holds shift[c] and the raw conv bias

    // fold BatchNorm (eval mode, eps 1e-5): y = conv(x)*scale + shift
    std::vector<double> scale(L.cout, 1.0), shift(L.cout, 0.0);
    for (int c = 0; c < L.cout && !plan; ++c) {
        if (bn) {
            const double g = bn[c], b = bn[L.cout + c], m = bn[2 * L.cout + c], v = bn[3 * L.cout + c];
            scale[c] = g / std::sqrt(v + 1e-5);
            shift[c] = b - m * scale[c];
        }
        if (conv_bias) shift[c] += conv_bias[c] * scale[c];
    }
    std::vector<float> bias(pc.nt * 16, 0.f);
    for (int c = 0; c < L.cout; ++c) bias[c] = (float)shift[c];
    if (plan) {
        std::vector<int32_t> m(bias.size(), -1);
        for (int c = 0; c < L.cout; ++c) m[c] = shift_at + c;
        plan_f32(std::move(m));
    }
    if ((rc = upload(pc, pc.bias, bias))) return rc;
    if (L.cout == 8 && pc.nt == 1) {   // pixel-pair kernels: rows 8-15 are the second pixel's 8 channels
        std::vector<float> b2(16);
        for (int c = 0; c < 16; ++c) b2[c] = (float)shift[c & 7];
        if (plan) {
            std::vector<int32_t> m(16);
            for (int c = 0; c < 16; ++c) m[c] = shift_at + (c & 7);
            plan_f32(std::move(m));
        }
        if ((rc = upload(pc, pc.bias_pair, b2))) return rc;
    }

    // The stem reads the paired-pixel (W+2)-wide volume written by stack_in: pixel p lives in the first half
    // of record p+2, so every x-offset of its taps is shifted by +2.
    const bool stem = (L.kd == 1 && L.kh == 9 && L.kw == 9 && L.dh == 2 && L.pd == 0 && L.ph == 8 && L.sh == 1 && L.cin == 3);
    // tap lists
    std::vector<std::vector<Tap>> tapsets;
    std::vector<std::pair<int, int>> phase;
    if (!L.transposed) {
        std::vector<Tap> taps;
        for (int kz = 0; kz < L.kd; ++kz)
            for (int ky = 0; ky < L.kh; ++ky)
                for (int kx = 0; kx < L.kw; ++kx)
                    taps.push_back(Tap{kz - L.pd, ky * L.dh - L.ph, kx * L.dw - L.pw + (stem ? 2 : 0), kz, ky, kx});
        tapsets.push_back(taps);
        phase.push_back({0, 0});
    } else {
        // out[oz,oy,ox] = sum in[iz,iy,ix] * w[kz,ky,kx] with oz = iz-1+kz, oy = 2*iy-1+ky, ox = 2*ix-1+kx.
        // For output parity p along a stride-2 axis (o = 2*g + p): p=0 uses k=1 at i=g; p=1 uses k=0 at
        // i=g+1 and k=2 at i=g.  Never materialise the zero-inserted input.
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
                std::vector<Tap> taps;
                for (int kz = 0; kz < 3; ++kz)
                    for (int ky = 0; ky < 3; ++ky) {
                        if ((ky & 1) == py) continue;  // py=0 -> ky odd only; py=1 -> ky even only
                        for (int kx = 0; kx < 3; ++kx) {
                            if ((kx & 1) == px) continue;
                            const int dy = (ky == 0) ? 1 : 0, dx = (kx == 0) ? 1 : 0;
                            taps.push_back(Tap{1 - kz, dy, dx, kz, ky, kx});
                        }
                    }
                tapsets.push_back(taps);
                phase.push_back({py, px});
            }
    }

    const int kvol = L.kd * L.kh * L.kw;
    auto wval = [&](int cout, int cin, const Tap &t) -> float {
        if (cin >= cin_own) {   // folded shortcut: its own weight on the centre tap (not scaled by this layer's BatchNorm)
            const int ce = cin - cin_own;
            return (ce < shortcut_cin && t.dz == 0 && t.dy == 0 && t.dx == 0) ? shortcut_w[(int64_t)cout * shortcut_cin + ce] : 0.f;
        }
        if (cin >= L.cin) return 0.f;
        const int64_t kidx = ((int64_t)t.kz * L.kh + t.ky) * L.kw + t.kx;
        const int64_t i = L.transposed ? ((int64_t)cin * L.cout + cout) * kvol + kidx : ((int64_t)cout * L.cin + cin) * kvol + kidx;
        if (plan) return weight[i];
        return (float)((double)weight[i] * scale[cout]);
    };

    // ---- first packing: the generic implicit-GEMM kernel, one launch per tap set: [KC][NT][part][64][8] --------------
    for (size_t vi = 0; vi < tapsets.size(); ++vi) {
        const auto &taps = tapsets[vi];
        Variant v;
        v.ooy = phase[vi].first;
        v.oox = phase[vi].second;
        v.ntaps = (int)taps.size();
        const int K8 = (int)taps.size() * c8n;
        v.KC = (K8 + 3) / 4;
        std::vector<TapEntry> tab(v.KC * 4);
        for (int k8 = 0; k8 < v.KC * 4; ++k8) {
            if (k8 < K8) {
                const Tap &t = taps[k8 / c8n];
                tab[k8] = TapEntry{t.dz, t.dy, t.dx, (k8 % c8n) * 8};
            } else {
                tab[k8] = TapEntry{0, 0, 0, -1};
            }
        }
        auto frag = [&](int f, int lane, int j) {
            const int cout = f % pc.nt * 16 + (lane & 15);
            const int k = f / pc.nt * 32 + (lane >> 4) * 8 + j;
            const int tapi = k / cin_pad;
            return cout < L.cout && tapi < (int)taps.size() ? wval(cout, k % cin_pad, taps[tapi]) : 0.f;
        };
        if ((rc = upload(pc, v.tab, tab)) || (rc = pack_frags(pc, v.wpk, prec, v.KC * pc.nt, frag))) return rc;
        pc.variants.push_back(v);
    }

    if (!L.transposed && L.kh == 1 && L.kw == 1 && L.cout <= 32 && L.cin <= 32) {
        std::vector<float> w32((size_t)L.kd * L.cin * L.cout);
        for (int kz = 0; kz < L.kd; ++kz)
            for (int ci = 0; ci < L.cin; ++ci)
                for (int co = 0; co < L.cout; ++co) w32[((size_t)kz * L.cin + ci) * L.cout + co] = wval(co, ci, Tap{0, 0, 0, kz, 0, 0});
        if (plan) {
            std::vector<int32_t> m(w32.size());
            for (size_t i = 0; i < w32.size(); ++i) m[i] = src_of(w32[i]);
            plan_f32(std::move(m));
        }
        if ((rc = upload(pc, pc.w32, w32))) return rc;
    }

    if (!L.transposed && L.bias && !bn && conv_bias && L.cout == 3 && L.kd == 1 && L.kh == 3 && L.kw == 3 && L.sh == 1 && L.ph == 1 && L.pw == 1 &&
        L.dh == 1 && L.cin % 8 == 0 && L.cin <= 64 && !shortcut_w) {
        std::vector<float> wh((size_t)3 * L.cin * 9 + 3);
        if (plan) {   // the raw weights (no BatchNorm: the folded ones are the same bits) and the raw bias
            std::vector<int32_t> m(wh.size());
            for (size_t i = 0; i < m.size(); ++i) m[i] = i < (size_t)n_w ? (int32_t)i : cbias_at + (int32_t)(i - n_w);
            plan_f32(std::move(m));
        } else {
            memcpy(wh.data(), weight, (size_t)3 * L.cin * 9 * sizeof(float));      // PyTorch (3, cin, 1, 3, 3) is already [c][ci][dy][dx]
            memcpy(wh.data() + (size_t)3 * L.cin * 9, conv_bias, 3 * sizeof(float));
        }
        if ((rc = upload(pc, pc.whead, wh))) return rc;
    }

    // ---- second packing for the LDS-tiled kernel, when a configuration covers this geometry ----------
    int geo = -1;
    if (L.transposed) geo = G3T;
    else if (L.kd == 3 && L.kh == 3 && L.kw == 3 && L.dh == 1 && L.pd == 1 && L.ph == 1 && L.sh == 1) geo = G3S1;
    else if (L.kd == 3 && L.kh == 3 && L.kw == 3 && L.dh == 1 && L.pd == 1 && L.ph == 1 && L.sh == 2) geo = G3S2;
    else if (L.kd == 1 && L.kh == 3 && L.kw == 3 && L.dh == 1 && L.pd == 0 && L.ph == 1 && L.sh == 1) geo = G2S1;
    else if (L.kd == 1 && L.kh == 3 && L.kw == 3 && L.dh == 1 && L.pd == 0 && L.ph == 1 && L.sh == 2) geo = G2S2;
    int cin_t = cin_pad;  // channels the tiled kernel contracts over (padding channels carry zero weights)
    if (stem) {
        // paired-pixel input (stack_in): record q = RGB(q-2) | RGB(q).  Taps (ky, jx) for jx in {0,2,4,6,8}
        // read record x+2*jx-6 and carry the weights of x-taps jx (channels 0..2) and jx+1 (channels
        // 4..6; zero for the non-existent tap 9).
        geo = G2D;
        cin_t = 8;
        tapsets.assign(1, std::vector<Tap>());
        for (int ky = 0; ky < 9; ++ky)
            for (int jx = 0; jx < 9; jx += 2) tapsets[0].push_back(Tap{0, 2 * ky - 8, 2 * jx - 6, 0, ky, jx});
    }
    auto wval_t = [&](int cout, int cin, const Tap &t) -> float {
        if (!stem) return wval(cout, cin, t);
        if ((cin & 3) == 3) return 0.f;
        Tap u = t;
        if (cin >= 4) {
            if (t.kx + 1 > 8) return 0.f;
            u.kx = t.kx + 1;
        }
        return wval(cout, cin & 3, u);
    };
    if (geo >= 0 && cin_t % 8 == 0) {
        int cg = (geo == G3S2 || geo == G2S2) ? 8 : (cin_t % 16 == 0 ? 16 : 8);
        // transposed conv: its 4 sub-pixel passes share one LDS image only when the whole contraction depth is
        // staged at once, so 32-channel groups (one fill instead of 4 x 2) where an instantiation exists
        if (geo == G3T && cin_t % 32 == 0 && tile_cfg_find(geo, pc.nt, 32)) cg = 32;
        // stride-(1,2,2) 3x3x3 over 64 channels (dres2.conv3): 16-channel stages on a 4 x 4 x 8 tile instead of eight 8-channel
        // stages on 5 x 4 x 16 (every stage re-fetches the 128-byte lines it takes a piece of): -18 %.  Measured on the 16- and
        // 32-channel stride-2 layers too: +25 % / +9 % SLOWER (smaller tile, more halo, 4-slice tiles on 10 slices) -- not used there.
        if (geo == G3S2 && cin_t % 64 == 0 && tile_cfg_find(geo, pc.nt, 16)) cg = 16;
        // per-slice 1x3x3 over 32 channels: ONE 32-channel stage per tile (each 128-byte pixel line is fetched once instead of
        // half of it per 16-channel stage -- the memory side moves whole 128-byte lines, profiles/r02_fetch_size_calibration.txt)
        if (geo == G2S1 && cin_t % 32 == 0 && tile_cfg_find(geo, pc.nt, 32)) cg = 32;   // +4..14 % on those layers
        // wide (8-wave, 640-point) tile wherever an instantiation exists (dffw_conv_tile.hip lists what was measured)
        // (the pack-time switches DFFW_NO_WIDE / DFFW_NO_CG32 / DFFW_NO_S2_CG16 / DFFW_STEM_NARROW / DFFW_NO_ROLL_PAIR / DFFW_NO_ROLL_T were retired in round 5: their
        // alternatives lost every A/B of rounds 1-4, profiles/r04_ab_forward_switches.txt and the rounds before)
        const bool wide = true;
        // pair: the stem's pixel-pair form (G2P) -- result rows 8-15 carry the filter as pixel x+2 sees the same records, and the
        // LDS image keeps only the footprint columns = 0,1 mod 4 (tap offsets in packed columns)
        auto pack_tile = [&](TilePack &tp, const TileCfg *cfg, int cg, bool pair) -> int {
            const GeoInfo gi = geo_info(cfg->geo);
            tp.cfg = cfg;
            tp.nstage = cin_t / cg;
            tp.npass = (int)tapsets.size();
            const int cg8 = cg / 8;
            for (int ps = 0; ps < tp.npass; ++ps) {
                // pair form (round 6): chunks 0-8 = filter row ky with the pair columns jx = 0, 2, 4, 6 as its four K octets, chunks 9-11 = the last pair column
                // (jx = 8) of rows 0-3, 4-7, 8.  Output rows y and y + 2 then read the SAME operand fragment for (y + 2, ky) and (y, ky + 1) -- the dilation is 2 --,
                // which stem_pipe loads once (its LDS port is the kernel's busiest unit: 0.65); conv_tile's pair-form kernel just follows the table
                std::vector<Tap> ptaps;
                if (pair && tapsets[ps].size() == 45) {
                    for (int ky = 0; ky < 9; ++ky)
                        for (int ji = 0; ji < 4; ++ji) ptaps.push_back(tapsets[ps][ky * 5 + ji]);
                    for (int ky = 0; ky < 9; ++ky) ptaps.push_back(tapsets[ps][ky * 5 + 4]);
                }
                const auto &taps = ptaps.empty() ? tapsets[ps] : ptaps;
                const int K8 = (int)taps.size() * cg8;
                const int KC = (K8 + 3) / 4;
                tp.KC[ps] = KC;
                tp.ntaps[ps] = (int)taps.size();
                tp.ooy[ps] = phase[ps].first;
                tp.oox[ps] = phase[ps].second;
                std::vector<int> tab(KC * 4, 0);
                for (int k8 = 0; k8 < K8; ++k8) {
                    const Tap &tpp = taps[k8 / cg8];
                    const int dzz = tpp.dz - gi.minz, dyy = tpp.dy - gi.miny, dxx = tpp.dx - gi.minx;
                    const int lx = pair ? dxx / 2 : ((gi.s == 2) ? ((dxx & 1) * (cfg->fxl / 2) + (dxx >> 1)) : dxx);
                    tab[k8] = ((dzz * cfg->fy + dyy) * cfg->fxl + lx) * (cg * 2) + (k8 % cg8) * 16;
                }
                // fragment f = (stage, KC chunk, output tile)
                auto frag = [&](int f, int lane, int j) {
                    const int cout = f % pc.nt * 16 + (lane & 15);
                    const int k = f / pc.nt % KC * 32 + (lane >> 4) * 8 + j;
                    const int tapi = k / cg, cin = f / pc.nt / KC * cg + k % cg;
                    if (tapi >= (int)taps.size()) return 0.f;
                    if (!pair) return cout < L.cout ? wval_t(cout, cin, taps[tapi]) : 0.f;
                    // row half h = pixel x + 2h: the record's pixels are filter columns (jx - h, jx + 1 - h) for it
                    const int h = (lane & 15) >> 3;
                    Tap u = taps[tapi];
                    u.kx += (cin >= 4 ? 1 : 0) - h;
                    return (cin & 3) != 3 && u.kx >= 0 && u.kx <= 8 ? wval(cout & 7, cin & 3, u) : 0.f;
                };
                if ((rc = upload(pc, tp.tab[ps], tab)) || (rc = pack_frags(pc, tp.wpk[ps], prec, tp.nstage * KC * pc.nt, frag))) return rc;
            }
            return DFFW_OK;
        };
        const TileCfg *cfg = tile_cfg_find(geo, pc.nt, cg, wide);
        if (cfg && cin_t % cg == 0 && (rc = pack_tile(pc.tile, cfg, cg, false))) return rc;
        // ... and on the 5 x 8 x 8 block where an instantiation exists (at most 4 output tiles per workgroup: wider layers always split there)
        if ((geo == G3S1 || geo == G3T) && cfg && cin_t % cg == 0 && L.cout >= 32 && !stem) {
            const TileCfg *ncfg = tile_cfg_find_shape(geo, std::min(pc.nt, 4), cg, 5, 8, 8);
            if (ncfg && (rc = pack_tile(pc.tile_narrow, ncfg, cg, false))) return rc;
        }
        const TileCfg *pcfg = (stem && L.cout == 8 && !getenv("DFFW_NO_STEM_PAIR")) ? tile_cfg_find(G2P, 1, 8, wide) : nullptr;
        if (pcfg && (rc = pack_tile(pc.tile_pair, pcfg, 8, true))) return rc;
    }
    // ---- third packing: conv_roll (rolling window along the slices) for the 16-channel 3x3x3 stride-1 layers ------
    // K order [dz][k5][32]: chunk k5 of a slice = in-slice taps 2*k5 and 2*k5+1 (tap 9 does not exist: zero weights),
    // lane group g -> tap 2*k5 + (g >> 1), channel octet g & 1
    if (geo == G3S1 && cin_pad == 16 && pc.nt == 1 && !stem) {
        pc.roll_pair = L.cout == 8;
        auto frag = [&](int c, int lane, int j) {
            const int row = lane & 15, gq = lane >> 4;
            const int cin = (gq & 1) * 8 + j;
            if (!pc.roll_pair) {
                const int tap9 = 2 * (c % 5) + (gq >> 1);
                return row < L.cout && tap9 < 9 ? wval(row, cin, tap_3x3x3(c / 5, tap9)) : 0.f;
            }
            // pixel pairs: result rows 0-7 = channels of the even pixel, 8-15 = of the odd one; chunk
            // (dz, ky, half) contracts input columns ix = 2*half + (gq >> 1) of the 4 the pair touches:
            // the even pixel sees ix as filter column kx = ix, the odd pixel as kx = ix - 1
            const int dz = c / 6, ky = (c % 6) / 2, half = c % 2;
            const int ix = 2 * half + (gq >> 1);
            const int cout = row & 7, kx = ix - (row >> 3);
            return cout < L.cout && kx >= 0 && kx <= 2 ? wval(cout, cin, tap_3x3x3(dz, 3 * ky + kx)) : 0.f;
        };
        if ((rc = pack_frags(pc, pc.wroll, prec, pc.roll_pair ? ROLL_CHUNKS_PAIR : ROLL_CHUNKS, frag))) return rc;
    }
    // ---- conv_rollx_k2 (dffw_conv_rollx.hip): 3x3x3 stride 1, 32 -> 16 channels (`dres3.conv0`): conv_roll's plain chunk order per 16-channel
    // input half: [half][dz][k5], K octet g = (tap 2*k5 + (g >> 1), channel half*16 + (g & 1)*8 ..)
    if (geo == G3S1 && cin_pad == 32 && L.cin == 32 && L.cout == 16 && !stem && !shortcut_w && prec == P_BF16X3) {
        auto frag = [&](int f, int lane, int j) {
            const int half = f / ROLL_CHUNKS, c = f % ROLL_CHUNKS, row = lane & 15, gq = lane >> 4;
            const int tap9 = 2 * (c % 5) + (gq >> 1);
            return row < L.cout && tap9 < 9 ? wval(row, half * 16 + (gq & 1) * 8 + j, tap_3x3x3(c / 5, tap9)) : 0.f;
        };
        if ((rc = pack_frags(pc, pc.wroll_k2, prec, 2 * ROLL_CHUNKS, frag))) return rc;
    }
    // ---- conv_slice32 (dffw_conv_slice.hip): per-slice 1x3x3, 32 -> 32 channels: chunk c = filter tap c ([ky][kx] order) x 32 channels (K octet g = channels 8g ..)
    // [chunk][output tile]
    if (geo == G2S1 && cin_pad == 32 && L.cin == 32 && L.cout == 32 && !shortcut_w && prec == P_BF16X3) {
        auto frag = [&](int f, int lane, int j) { return wval(f % 2 * 16 + (lane & 15), (lane >> 4) * 8 + j, tap_1x3x3(f / 2)); };
        if ((rc = pack_frags(pc, pc.wslice32, prec, SLICE32_CHUNKS * 2, frag))) return rc;
    }
    // ---- conv_slice64 (dffw_conv_slice.hip): per-slice 1x3x3, 64 -> 64 channels: wave share = one 16-channel output tile; chunk c = (filter tap c / 2, channel half c % 2),
    // K octet g = channels 32 (c % 2) + 8g ..
    if (geo == G2S1 && cin_pad == 64 && L.cin == 64 && L.cout == 64 && !shortcut_w && prec == P_BF16X3) {
        auto frag = [&](int f, int lane, int j) {
            const int nt = f / SLICE64_CHUNKS, c = f % SLICE64_CHUNKS;
            return wval(nt * 16 + (lane & 15), (c % 2) * 32 + (lane >> 4) * 8 + j, tap_1x3x3(c / 2));
        };
        if ((rc = pack_frags(pc, pc.wslice64, prec, 4 * SLICE64_CHUNKS, frag))) return rc;
    }
    // ... and its HEAD variant for the level-3 alignment head's first conv over [features 32 | flow 2 | pad 6] records: chunk c < 9 = tap c x the 32 feature channels;
    // chunk 9 + k: K octet g = the record's fifth channel octet (flow_x, flow_y, zeros) at tap 4k + g (taps 9 .. 11: zero weights)
    if (geo == G2S1 && cin_pad == 40 && L.cin == 34 && L.cout == 64 && !shortcut_w && prec == P_BF16X3) {
        auto frag = [&](int f, int lane, int j) {
            const int nt = f / SLICE64_HEAD_CHUNKS, c = f % SLICE64_HEAD_CHUNKS, gq = lane >> 4;
            const int tap = c < 9 ? c : 4 * (c - 9) + gq, cin = c < 9 ? gq * 8 + j : 32 + j;
            return tap < 9 && cin < L.cin ? wval(nt * 16 + (lane & 15), cin, tap_1x3x3(tap)) : 0.f;
        };
        if ((rc = pack_frags(pc, pc.wslice64, prec, 4 * SLICE64_HEAD_CHUNKS, frag))) return rc;
    }
    // ... and its CAT variant (conv_slice32_cat): 32 -> 32 over t with the block's folded 1x1x1 shortcut over x: chunks 0-8 = the taps over t, chunk 9 = the centre tap
    // over the shortcut's 32 channels (channels 32 .. 63 of the virtual concat)
    if (geo == G2S1 && cin_own == 32 && shortcut_w && shortcut_cin == 32 && L.cout == 32 && prec == P_BF16X3) {
        auto frag = [&](int f, int lane, int j) {
            const int nt = f / SLICE32_CAT_CHUNKS, c = f % SLICE32_CAT_CHUNKS;
            return wval(nt * 16 + (lane & 15), (c < 9 ? 0 : 32) + (lane >> 4) * 8 + j, tap_1x3x3(c < 9 ? c : 4));
        };
        if ((rc = pack_frags(pc, pc.wslice64, prec, 2 * SLICE32_CAT_CHUNKS, frag))) return rc;
        pc.slice_cat = true;
    }
    // ---- conv_rollk (dffw_conv_rollk.hip): 3x3x3 stride 1, 32 / 64 -> 32 / 64 channels, the contraction split over the workgroup's waves: wave w =
    // (16-channel group w >> 1, tap half w & 1); tap slot s of a half = filter tap 14 * (w & 1) + s in [dz][ky][kx] order (tap 27: zero weights);
    // chunk c = slots 2c, 2c + 1; K octet g = (slot 2c + (g >> 1), channel octet g & 1 of the group)
    if (geo == G3S1 && (cin_pad == 32 || cin_pad == 64) && L.cin == cin_pad && L.cout % 32 == 0 && L.cout <= 64 && !stem && !shortcut_w && prec == P_BF16X3) {
        const int nw = cin_pad / 8, npair = L.cout / 32;
        // fragment f = (output pair, wave, chunk, output tile)
        auto frag = [&](int f, int lane, int j) {
            const int nt = f % 2, c = f / 2 % ROLLK_CHUNKS, wv = f / (2 * ROLLK_CHUNKS) % nw, op = f / (2 * ROLLK_CHUNKS * nw);
            const int gq = lane >> 4;
            const int tap = (wv & 1) * 2 * ROLLK_CHUNKS + 2 * c + (gq >> 1);
            const int cin = (wv >> 1) * 16 + (gq & 1) * 8 + j;
            return tap < 27 ? wval((op * 2 + nt) * 16 + (lane & 15), cin, tap_3x3x3(tap / 9, tap % 9)) : 0.f;
        };
        if ((rc = pack_frags(pc, pc.wrollk, prec, npair * nw * ROLLK_CHUNKS * 2, frag))) return rc;
    }
    // ---- conv_rollt (dffw_conv_rollt.hip): transposed 3x3x3 s(1,2,2), 32 / 64 -> 32 / 64 channels, the filter split over the workgroup's waves by output phase
    // and 16-channel output tile (rollt::Prog<role>: the wave's operand fragment sets and the accumulator slots = output phases each feeds).  A weight unit =
    // one tap x 32 channels (K octet g = channels 32 chunk + 8 g ..) x 16 outputs; units in the wave's set order, one per fed slot
    if (geo == G3T && (cin_pad == 32 || cin_pad == 64 || (cin_pad == 16 && L.cout == 16)) && L.cin == cin_pad &&
        ((L.cout % 32 == 0 && L.cout <= 64) || (L.cout == 16 && cin_pad <= 32)) && !shortcut_w && prec == P_BF16X3) {
        // (16 output channels, the wide form: the shares of the roles A32 / C32 once -- "waves" 0, 1 of one "half")
        const int nw = L.cout == 16 ? 2 : cin_pad / 8, nhalf = L.cout == 16 ? 1 : L.cout / 32;
        struct Unit {
            int cout0 = -1, chunk = 0;   // cout0 < 0: a unit slot the wave does not use (zero weights)
            Tap tap{};
        };
        std::vector<Unit> units((size_t)nhalf * nw * rollt::MAXU);   // [half][wave][unit]
        auto list_role = [&](auto ROLE_, int oh, int wv) {
            using PR = rollt::Prog<decltype(ROLE_)::value>;
            Unit *un = &units[((size_t)oh * nw + wv) * rollt::MAXU];
            const int cout0 = (oh * 2 + ((wv >> 1) & 1)) * 16;
            for (int i = 0; i < PR::NS; ++i) {
                int u = PR::ubase(i);
                for (int sl = 0; sl < PR::NACC; ++sl) {
                    if (!((PR::feeds(i) >> sl) & 1)) continue;
                    const int ph = PR::phase(sl), py = ph >> 1, px = ph & 1, d = PR::d(i), dy = PR::dy(i), dx = PR::dx(i);
                    un[u++] = Unit{cout0, PR::chunk(i), Tap{d - 1, dy, dx, 2 - d, rollt::tap_of(py, dy), rollt::tap_of(px, dx)}};
                }
            }
        };
        for (int oh = 0; oh < nhalf; ++oh)
            for (int wv = 0; wv < nw; ++wv)
                switch (rollt_role(cin_pad == 16 ? 32 : cin_pad, wv)) {
                    case rollt::R_A: list_role(std::integral_constant<int, rollt::R_A>{}, oh, wv); break;
                    case rollt::R_B: list_role(std::integral_constant<int, rollt::R_B>{}, oh, wv); break;
                    case rollt::R_C: list_role(std::integral_constant<int, rollt::R_C>{}, oh, wv); break;
                    case rollt::R_D: list_role(std::integral_constant<int, rollt::R_D>{}, oh, wv); break;
                    case rollt::R_A32: list_role(std::integral_constant<int, rollt::R_A32>{}, oh, wv); break;
                    default: list_role(std::integral_constant<int, rollt::R_C32>{}, oh, wv); break;
                }
        auto frag = [&](int f, int lane, int j) {
            const Unit &un = units[f];
            return un.cout0 >= 0 ? wval(un.cout0 + (lane & 15), un.chunk * 32 + (lane >> 4) * 8 + j, un.tap) : 0.f;
        };
        if ((rc = pack_frags(pc, pc.wrollt, prec, (int)units.size(), frag))) return rc;
    }
    // The attention fragments below do not follow the common layout: their 1x1x1 forms carry a low half for j < 4 only, and the
    // 32-channel form interleaves parts with output tiles.  put() splits one value into wr[hi_at] and, where the form has one, wr[lo_at].
    auto put = [&](std::vector<uint16_t> &wr, size_t hi_at, size_t lo_at, bool has_lo, float val) {
        if (plan) {   // one entry per 16-bit slot: 2 * source + part
            const int32_t src = src_of(val);
            t_next.kind = RK_SLOTS;
            if (t_next.map.size() != wr.size()) t_next.map.assign(wr.size(), -1);
            t_next.map[hi_at] = src < 0 ? -1 : 2 * src;
            if (parts == 2 && has_lo) t_next.map[lo_at] = src < 0 ? -1 : 2 * src + 1;
            return;
        }
        uint16_t hi, lo;
        host_split(prec, val, hi, lo);
        wr[hi_at] = hi;
        if (parts == 2 && has_lo) wr[lo_at] = lo;
    };
    // ---- srd_roll stage C: the attention convs of the 8-channel SRD block (DEN.py:322-323) in pixel-pair form.  Result row
    // m = (pixel m >> 3 of the pair, channel m & 7).  3x1x1: chunk 0 K octet g = (pixel g >> 1, slice g & 1), chunk 1 = slice 2 in the
    // 1x1x1 form (its operand is what stage B of the same step leaves in registers).  1x1x1: K octet g = (pixel g >> 1, input channels 4*(g & 1)..+3 as [hi x4 | lo x4] of the split
    // operand): fragment 0 carries w_hi against both halves (w_hi*a_hi + w_hi*a_lo), fragment 1 w_lo against the hi half.
    if (!L.transposed && L.kh == 1 && L.kw == 1 && L.cin == 8 && L.cout == 8 && !bn && !conv_bias && (L.kd == 3 || L.kd == 1)) {
        std::vector<uint16_t> wr((size_t)(L.kd == 3 ? 2 * parts : parts) * 512, 0);
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
                const int row = lane & 15, gq = lane >> 4, px = row >> 3, co = row & 7;
                const bool mine = (gq >> 1) == px;
                const size_t e = (size_t)lane * 8 + j;
                if (L.kd == 3) {
                    put(wr, e, 512 + e, true, mine ? wval(co, j, Tap{0, 0, 0, gq & 1, 0, 0}) : 0.f);
                    // chunk 1 = slice tap 2 against the operand stage B leaves in registers (the 1x1x1 form below)
                    put(wr, parts * 512 + e, (parts + 1) * 512 + e, j < 4, mine ? wval(co, 4 * (gq & 1) + (j & 3), Tap{0, 0, 0, 2, 0, 0}) : 0.f);
                } else {
                    put(wr, e, 512 + e, j < 4, mine ? wval(co, 4 * (gq & 1) + (j & 3), Tap{0, 0, 0, 0, 0, 0}) : 0.f);
                }
            }
        if ((rc = upload(pc, pc.watt, wr))) return rc;
    }
    // the same for the 16-channel block (srd_roll16, no pixel pairs: result row = channel).  3x1x1: chunk 0 K octet g =
    // (slice g >> 1, channel octet g & 1), chunk 1 = slice 2 in the 1x1x1 form.  1x1x1: K octet g = input channels 4g..4g+3 as
    // [hi x4 | lo x4]; fragment 0 = w_hi against both halves, fragment 1 = w_lo against the hi half.
    if (!L.transposed && L.kh == 1 && L.kw == 1 && L.cin == 16 && L.cout == 16 && !bn && !conv_bias && (L.kd == 3 || L.kd == 1)) {
        std::vector<uint16_t> wr((size_t)(L.kd == 3 ? 2 * parts : parts) * 512, 0);
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
                const int co = lane & 15, gq = lane >> 4;
                const size_t e = (size_t)lane * 8 + j;
                if (L.kd == 3) {
                    put(wr, e, 512 + e, true, wval(co, (gq & 1) * 8 + j, Tap{0, 0, 0, gq >> 1, 0, 0}));
                    // chunk 1 = slice tap 2 against the operand stage B leaves in registers (the 1x1x1 form below)
                    put(wr, parts * 512 + e, (parts + 1) * 512 + e, j < 4, wval(co, 4 * gq + (j & 3), Tap{0, 0, 0, 2, 0, 0}));
                } else {
                    put(wr, e, 512 + e, j < 4, wval(co, 4 * gq + (j & 3), Tap{0, 0, 0, 0, 0, 0}));
                }
            }
        if ((rc = upload(pc, pc.watt, wr))) return rc;
    }
    // the same for the 32-channel block (srd_attention_mfma, two 16-channel output tiles).  3x1x1: chunk k = slice k, K octet g =
    // input channels 8g..8g+7.  1x1x1: channel chunk c = input channels 16c..16c+15, K octet g = channels 16c+4g..+3 as [hi | lo].
    if (!L.transposed && L.kh == 1 && L.kw == 1 && L.cin == 32 && L.cout == 32 && !bn && !conv_bias && L.kd == 3) {
        // [slice][output tile]: the common layout
        auto frag = [&](int f, int lane, int j) { return wval(f % 2 * 16 + (lane & 15), (lane >> 4) * 8 + j, Tap{0, 0, 0, f / 2, 0, 0}); };
        if ((rc = pack_frags(pc, pc.watt, prec, 3 * 2, frag))) return rc;
    }
    if (!L.transposed && L.kh == 1 && L.kw == 1 && L.cin == 32 && L.cout == 32 && !bn && !conv_bias && L.kd == 1) {
        // [channel chunk][part][output tile]
        std::vector<uint16_t> wr((size_t)2 * parts * 2 * 512, 0);
        for (int nt = 0; nt < 2; ++nt)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j)
                    for (int c = 0; c < 2; ++c) {
                        const size_t e = (size_t)lane * 8 + j;
                        put(wr, ((size_t)(c * parts) * 2 + nt) * 512 + e, ((size_t)(c * parts + 1) * 2 + nt) * 512 + e, j < 4,
                            wval(nt * 16 + (lane & 15), 16 * c + 4 * (lane >> 4) + (j & 3), Tap{0, 0, 0, 0, 0, 0}));
                    }
        if ((rc = upload(pc, pc.watt, wr))) return rc;
    }
    // ---- of_roll (alignment network, stride-1 blocks): conv.0 with 8 (3 real) input channels -> 16: chunk k, K octet g = tap 4k + g;
    // conv.2 16 -> 16 with the block's 1x1x1 shortcut folded in (shortcut_w): 5 chunks over t as below + ONE chunk whose K octet g
    // = channel octet g of the block input at the centre tap
    if (geo == G2S1 && cin_pad == 8 && L.cout == 16 && !shortcut_w) {
        auto frag = [&](int c, int lane, int j) {
            const int tap = 4 * c + (lane >> 4);
            return tap < 9 ? wval(lane & 15, j, tap_1x3x3(tap)) : 0.f;
        };
        if ((rc = pack_frags(pc, pc.wsrd, prec, 3, frag))) return rc;
    }
    // of_roll8: conv.2 8 -> 8 with the folded shortcut, pixel-pair form: chunk ky as for srd_roll (K octet g = input column 2*pair + g),
    // chunk 3 = shortcut: K octet g < 2 = the 8 block-input channels of pixel 2*pair + g, seen only by that pixel's result rows
    if (geo == G2S1 && cin_own == 8 && L.cout == 8 && shortcut_w && shortcut_cin <= 8) {
        auto frag = [&](int c, int lane, int j) {
            const int row = lane & 15, gq = lane >> 4, cout = row & 7, px = row >> 3;
            if (c == 3) return gq == px && j < shortcut_cin ? wval(cout, cin_own + j, tap_1x3x3(4)) : 0.f;
            const int kx = gq - px;
            return kx >= 0 && kx <= 2 ? wval(cout, j, tap_1x3x3(3 * c + kx)) : 0.f;
        };
        if ((rc = pack_frags(pc, pc.wsrd, prec, 4, frag))) return rc;
    }
    if (geo == G2S1 && cin_own == 16 && L.cout == 16 && shortcut_w && (shortcut_cin + 7) / 8 * 8 <= 16) {
        auto frag = [&](int c, int lane, int j) {
            const int co = lane & 15, gq = lane >> 4;
            if (c == 5) return gq * 8 + j < shortcut_cin ? wval(co, cin_own + gq * 8 + j, tap_1x3x3(4)) : 0.f;
            const int tap = 2 * c + (gq >> 1);
            return tap < 9 ? wval(co, (gq & 1) * 8 + j, tap_1x3x3(tap)) : 0.f;
        };
        if ((rc = pack_frags(pc, pc.wsrd, prec, OF_CHUNKS_B, frag))) return rc;
    }
    // ---- head_warp<CF = 16>: the [cur (16) | flow (2)] part of the level-2 alignment head's first conv, 32 output channels: chunk k,
    // K octet g = o = 4k + g -> (filter tap o / 3, channel octet o % 3) of the 24-channel records the kernel builds in LDS
    // [chunk][output tile]
    if (geo == G2S1 && L.cin == 18 && cin_pad == 24 && L.cout == 32 && !shortcut_w) {
        auto frag = [&](int f, int lane, int j) {
            const int o = 4 * (f / 2) + (lane >> 4);
            return o < 27 ? wval(f % 2 * 16 + (lane & 15), o % 3 * 8 + j, tap_1x3x3(o / 3)) : 0.f;
        };
        if ((rc = pack_frags(pc, pc.wsrd, prec, head_warp_chunks(16) * 2, frag))) return rc;
    }
    // ---- of_s2 (down-sampling block 8 -> 16 of the alignment network): conv.0 = 1x3x3 stride (1,2,2), 8 -> 16: chunk k, K octet g = filter
    // tap 4k + g; its 1x1x1 stride-2 shortcut (no BatchNorm, no bias): one chunk, K octet 0 = the 8 input channels
    if (geo == G2S2 && cin_pad == 8 && L.cout == 16 && !shortcut_w) {
        auto frag = [&](int c, int lane, int j) {
            const int tap = 4 * c + (lane >> 4);
            return tap < 9 ? wval(lane & 15, j, tap_1x3x3(tap)) : 0.f;
        };
        if ((rc = pack_frags(pc, pc.wsrd, prec, 3, frag))) return rc;
    }
    if (!L.transposed && L.kd == 1 && L.kh == 1 && L.kw == 1 && L.sh == 2 && cin_pad == 8 && L.cout == 16 && !bn && !conv_bias && !shortcut_w) {
        auto frag = [&](int, int lane, int j) { return lane < 16 ? wval(lane, j, Tap{0, 0, 0, 0, 0, 0}) : 0.f; };   // K octet 0 only
        if ((rc = pack_frags(pc, pc.wsrd, prec, 1, frag))) return rc;
    }
    // ---- srd_roll16: the per-slice 1x3x3 16 -> 16 convs: chunk k, K octet g = (filter tap 2k + (g >> 1), channel octet g & 1)
    // (packed with a sixth, all-zero chunk: the same buffer then serves as the second conv of of_roll_kernel, whose shortcut chunk
    // it leaves empty, for plain conv -> conv chains such as the alignment heads' .2.0 -> .4.0)
    if (geo == G2S1 && cin_pad == 16 && L.cout == 16 && !shortcut_w) {
        auto frag = [&](int c, int lane, int j) {
            const int gq = lane >> 4, tap = 2 * c + (gq >> 1);
            return c < SRD16_CHUNKS && tap < 9 ? wval(lane & 15, (gq & 1) * 8 + j, tap_1x3x3(tap)) : 0.f;
        };
        if ((rc = pack_frags(pc, pc.wsrd, prec, OF_CHUNKS_B, frag))) return rc;
    }
    // ---- srd_roll: the per-slice 1x3x3 8 -> 8 convs of the fused SRD block, in pixel-pair form: chunk = filter row ky;
    // result rows 0-7 = channels of the even pixel of a pair, rows 8-15 = of the odd one; K octet g = input column 2*pair + g,
    // which the even pixel sees as filter column g and the odd pixel as filter column g - 1
    if (geo == G2S1 && cin_pad == 8 && L.cout == 8 && !shortcut_w) {
        auto frag = [&](int c, int lane, int j) {
            const int row = lane & 15, kx = (lane >> 4) - (row >> 3);
            return kx >= 0 && kx <= 2 ? wval(row & 7, j, tap_1x3x3(3 * c + kx)) : 0.f;
        };
        if ((rc = pack_frags(pc, pc.wsrd, prec, SRD_CHUNKS, frag))) return rc;
    }
    // ---- conv_roll_efd: 3x3x3 8 -> 16 (stride 1 on the pooled volume, or stride (1,2,2)): chunk (dz, k3), K octet g = tap 4*k3 + g
    if ((geo == G3S1 || geo == G3S2) && cin_pad == 8 && L.cout == 16 && !shortcut_w) {
        auto frag = [&](int c, int lane, int j) {
            const int tap = 4 * (c % 3) + (lane >> 4);
            return tap < 9 ? wval(lane & 15, j, tap_3x3x3(c / 3, tap)) : 0.f;
        };
        if ((rc = pack_frags(pc, pc.wroll8, prec, ROLL_CHUNKS_8, frag))) return rc;
    }
    // ---- conv_roll_s2: 3x3x3 stride (1,2,2), 16 / 32 -> 16 / 32 / 64 channels: per (16-channel output tile, 16-channel input half) 15 chunks
    // [dz][k5], K octet g = (in-slice tap 2*k5 + (g >> 1), channel octet g & 1 of the half), as conv_roll's plain form
    // (the same order for the stride-1 16 -> 32 layer `FM_conv2.0.max_pooling.1`: the pooled branch of conv_efd16)
    const bool pool15 = geo == G3S1 && cin_pad == 16 && L.cout == 32 && !shortcut_w && !stem;
    if ((geo == G3S2 && (cin_pad == 16 || cin_pad == 32) && L.cout % 16 == 0 && L.cout <= 64 && !(cin_pad == 16 && L.cout == 64) && !shortcut_w) || pool15) {
        const int ntl = L.cout / 16, khn = cin_pad / 16;
        // fragment f = (output tile, input half, chunk)
        auto frag = [&](int f, int lane, int j) {
            const int c = f % ROLL_CHUNKS, kh = f / ROLL_CHUNKS % khn, nt = f / ROLL_CHUNKS / khn, gq = lane >> 4;
            const int tap9 = 2 * (c % 5) + (gq >> 1);
            return tap9 < 9 ? wval(nt * 16 + (lane & 15), kh * 16 + (gq & 1) * 8 + j, tap_3x3x3(c / 5, tap9)) : 0.f;
        };
        if ((rc = pack_frags(pc, pool15 ? pc.wroll15 : pc.wroll_s2, prec, ntl * khn * ROLL_CHUNKS, frag))) return rc;
    }
    // ---- conv_roll_t32: transposed 3x3x3 s(1,2,2), 32 -> 16 channels, one fragment set per output row phase py.  A chunk = one
    // tap x 32 channels (K octet g = channel octet g).  Enumeration (must match the kernel): x phase 0 first: (window slice d,
    // row tap rt) with filter column 1 at input column x; then x phase 1: (d, rt, ct): ct = 0 -> filter column 2 at x, ct = 1 ->
    // filter column 0 at x+1.  Row taps: py = 0: filter row 1 at input row y; py = 1: rt = 0 -> filter row 2 at y, rt = 1 -> row 0 at y+1.
    if (geo == G3T && (cin_pad == 32 || cin_pad == 16) && L.cout == 16) {   // (16 input channels: octets 2, 3 get zero weights)
        auto frag = [&](int f, int lane, int j) {
            const int py = f >= ROLL_CHUNKS_T32_0, c = py ? f - ROLL_CHUNKS_T32_0 : f;
            const int nrow = py ? 2 : 1, nch0 = 3 * nrow, e = c - nch0;
            const int d = c < nch0 ? c / nrow : e / (2 * nrow);
            const int rt = c < nch0 ? c % nrow : (e / 2) % nrow;
            const int ct = c < nch0 ? 0 : e % 2;
            const int ky = py ? (rt == 0 ? 2 : 0) : 1, dy = (py && rt == 1) ? 1 : 0;
            const int kx = c < nch0 ? 1 : (ct == 0 ? 2 : 0), dx = ct;
            const int cin = (lane >> 4) * 8 + j;
            return cin < cin_pad ? wval(lane & 15, cin, Tap{d - 1, dy, dx, 2 - d, ky, kx}) : 0.f;
        };
        if ((rc = pack_frags(pc, pc.wroll_t32, prec, ROLL_CHUNKS_T32_0 + ROLL_CHUNKS_T32_1, frag))) return rc;
    }
    // ---- conv_roll_t: transposed 3x3x3 s(1,2,2), 16 -> 8 channels.  Result rows 0-7 = output pixel 2x, rows 8-15 = pixel
    // 2x+1; chunk c < 3: output row phase py = 0 (filter row 1 at input row y), slice c of the window; c >= 3: py = 1,
    // slice (c-3)/2, filter row 2 at input row y ((c-3) even) or filter row 0 at input row y+1 (odd).  Lane group g
    // contracts input column x + (g >> 1), channel octet g & 1: pixel 2x sees only column x (filter column 1), pixel 2x+1
    // sees column x (filter column 2) and column x+1 (filter column 0).  Window slice d is input slice oz-1+d = filter slice 2-d.
    if (geo == G3T && cin_pad == 16 && L.cout == 8) {
        auto frag = [&](int c, int lane, int j) {
            const int row = lane & 15, gq = lane >> 4;
            const int cout = row & 7, px = row >> 3, dx = gq >> 1, cin = (gq & 1) * 8 + j;
            const int d = c < 3 ? c : (c - 3) / 2;
            const bool down = c >= 3 && ((c - 3) & 1);
            const int ky = c < 3 ? 1 : (down ? 0 : 2), dy = down ? 1 : 0;
            int kx = -1;
            if (px == 0 && dx == 0) kx = 1;
            if (px == 1) kx = dx == 0 ? 2 : 0;
            return kx >= 0 ? wval(cout, cin, Tap{d - 1, dy, dx, 2 - d, ky, kx}) : 0.f;
        };
        if ((rc = pack_frags(pc, pc.wroll_t, prec, ROLL_CHUNKS_T, frag))) return rc;
    }
    return DFFW_OK;
}

int plan_conv(const LayerDef &def, int prec, int shortcut_cin, LayerPlan &out) {
    out = LayerPlan();
    out.n_w = (int64_t)def.cin * def.cout * def.kd * def.kh * def.kw;
    out.n_sc = shortcut_cin > 0 ? (int64_t)def.cout * shortcut_cin : 0;
    out.cout = def.cout;
    out.has_bias = def.bias;
    if (out.scratch_floats() >= (1 << 30)) return dffw_fail(DFFW_EINVAL, "plan_conv: layer %s is too large for 31-bit source indices", def.conv.c_str());
    std::vector<float> probe((size_t)(out.n_w + out.n_sc));
    for (size_t i = 0; i < probe.size(); ++i) {
        const uint32_t u = (uint32_t)i + 1;
        memcpy(&probe[i], &u, 4);
    }
    const float present = 0.f;   // bn / conv_bias are not read in plan mode: only whether the layer has them
    PackedConv tmp;
    t_next = BufPlan();
    t_plan = &out;
    const int rc = pack_conv(def, prec, probe.data(), def.bn.empty() ? nullptr : &present, def.bias ? &present : nullptr, tmp,
                             out.n_sc ? probe.data() + out.n_w : nullptr, shortcut_cin);
    t_plan = nullptr;
    t_next = BufPlan();
    if (rc) return rc;
    const int64_t n_src = out.scratch_floats();
    for (const BufPlan &b : out.bufs)
        for (int32_t m : b.map)
            if (m < -1 || (b.kind == RK_SLOTS ? m >> 1 : m) >= n_src)
                return dffw_fail(DFFW_EINVAL, "plan_conv: layer %s has a source index outside its %lld sources", def.conv.c_str(), (long long)n_src);
    return DFFW_OK;
}

// conv over [ref | cur | flow] = conv_ref(ref) + conv_cur([cur | flow]) (linearity): the ref part is the same for
// every slice of a sample, so it is computed once per sample and added as a slice-broadcast residual
int pack_head_split(const LayerDef &L, int prec, const float *weight, const float *bn, PackedConv &ref, PackedConv &cur) {
    const int C = L.head_split, kv = L.kd * L.kh * L.kw;
    auto slice = [&](int c0, int c1) {
        std::vector<float> ws((size_t)L.cout * (c1 - c0) * kv);
        for (int co = 0; co < L.cout; ++co)
            memcpy(ws.data() + (size_t)co * (c1 - c0) * kv, weight + ((size_t)co * L.cin + c0) * kv, (size_t)(c1 - c0) * kv * sizeof(float));
        return ws;
    };
    LayerDef Lr = L, Lc = L;
    Lr.conv = L.conv + "#ref"; Lr.cin = C; Lr.head_split = 0;
    Lc.conv = L.conv + "#cur"; Lc.cin = L.cin - C; Lc.head_split = 0;
    std::vector<float> bn_scale_only(bn, bn + 4 * (size_t)L.cout);   // gamma | beta | mean | var with beta = mean = 0: no shift
    for (int c = 0; c < L.cout; ++c) bn_scale_only[L.cout + c] = bn_scale_only[2 * L.cout + c] = 0.f;
    const std::vector<float> wr = slice(0, C), wc = slice(C, L.cin);
    if (int rc = pack_conv(Lr, prec, wr.data(), bn_scale_only.data(), nullptr, ref)) return rc;
    return pack_conv(Lc, prec, wc.data(), bn, nullptr, cur);
}

}  // namespace dffw
