// Repacking conv weights on the GPU: the C ABI of the kernels of dffw_repack.hip.  dffw_engine_update resolves every parameter the
// live layers need before anything is launched, builds the engine's repack plan at its first call (dffw_pack.cpp's plan mode: one source map per
// packed buffer, one scratch per packed layer, one static gather job table) and from then on only enqueues: the fold launches, whose layer tables
// are their kernel arguments, and one gather launch over all buffers of all layers.
#include <map>
#include <memory>

#include "dffw_repack.h"
#include "dffw_run.h"

namespace dffw {

void free_repack_plan(RepackPlan *p) {
    if (!p) return;
    for (void *q : p->owned) (void)hipFree(q);
    delete p;
}

namespace {

int64_t up256(int64_t n) { return (n + 255) & ~(int64_t)255; }

// Builds e->repack: the plan of every packed layer (it must describe exactly the buffers the engine holds), the source maps and the job table on
// the device.  Allocates and copies; leaves the engine as it was when it fails.
int build_plan(dffw_engine *e) {
    std::unique_ptr<RepackPlan, void (*)(RepackPlan *)> P(new RepackPlan, free_repack_plan);
    const std::vector<LayerDef> &table = net_layers(e->net);
    std::map<std::string, int> cin_of;
    for (const LayerDef &L : table) cin_of[L.conv] = L.cin;
    int64_t map_bytes = 0, n_jobs = 0;
    for (auto &kv : e->convs) {
        const PackedConv &pc = kv.second;
        RepackLayer rl;
        rl.name = kv.first;
        int scin = 0;
        if (!pc.def.shortcut.empty()) {
            auto it = cin_of.find(pc.def.shortcut);
            if (it == cin_of.end()) return fail(DFFW_EINVAL, "repack plan: layer %s folds an unknown shortcut %s", kv.first.c_str(), pc.def.shortcut.c_str());
            scin = it->second;
        }
        int rc = plan_conv(pc.def, e->prec, scin, rl.plan);
        if (rc) return rc;
        if (pc.def.cout > FOLD_MAX_COUT) return fail(DFFW_EINVAL, "repack plan: layer %s has %d output channels, the fold kernel holds %d", kv.first.c_str(), pc.def.cout, FOLD_MAX_COUT);
        if (rl.plan.bufs.size() != pc.owned.size() || pc.owned.size() != pc.owned_bytes.size())
            return fail(DFFW_EINVAL, "repack plan: layer %s would pack %zu buffers, the engine holds %zu (a DFFW_* packing switch changed since the engine was built?)",
                        kv.first.c_str(), rl.plan.bufs.size(), pc.owned.size());
        for (size_t i = 0; i < pc.owned.size(); ++i) {
            const BufPlan &b = rl.plan.bufs[i];
            if (b.bytes != pc.owned_bytes[i])
                return fail(DFFW_EINVAL, "repack plan: buffer %zu of layer %s would be %zu bytes, the engine holds %zu", i, kv.first.c_str(), b.bytes, pc.owned_bytes[i]);
            const size_t parts = (size_t)prec_parts(e->prec);
            const bool fits = b.kind == RK_CONST ? b.map.empty()
                              : b.kind == RK_FRAGS ? (b.map.size() * 2 * parts == b.bytes && b.map.size() % 512 == 0)
                              : b.kind == RK_SLOTS ? (b.map.size() * 2 == b.bytes && b.map.size() % 8 == 0)
                                                   : b.map.size() * 4 == b.bytes;
            if (!fits) return fail(DFFW_EINVAL, "repack plan: the source map of buffer %zu of layer %s does not cover its %zu bytes", i, kv.first.c_str(), b.bytes);
            if (b.kind != RK_CONST) {
                map_bytes += up256((int64_t)b.map.size() * 4);
                ++n_jobs;
                P->map_bytes += (int64_t)b.map.size() * 4;
                P->buffer_bytes += (int64_t)b.bytes;
            }
        }
        P->fold_bytes += 2 * rl.plan.scratch_floats() * 4;
        rl.scratch_off = P->scratch_floats;
        P->scratch_floats += (rl.plan.scratch_floats() + 63) & ~(int64_t)63;
        P->layers.push_back(std::move(rl));
    }
    if (P->scratch_floats >= ((int64_t)1 << 31) || n_jobs == 0) return fail(DFFW_EINVAL, "repack plan: %lld scratch floats, %lld buffers", (long long)P->scratch_floats, (long long)n_jobs);

    auto dev_alloc = [&](void **p, int64_t bytes) -> hipError_t {
        hipError_t h = hipMalloc(p, (size_t)bytes);
        if (h == hipSuccess) {
            P->owned.push_back(*p);
            P->device_bytes += bytes;
        }
        return h;
    };
    char *maps = nullptr;
    HIPCHK(dev_alloc((void **)&P->scratch, P->scratch_floats * 4));
    HIPCHK(dev_alloc((void **)&maps, map_bytes));
    HIPCHK(dev_alloc((void **)&P->jobs, n_jobs * (int64_t)sizeof(GatherJob)));
    HIPCHK(hipMemset(P->scratch, 0, (size_t)P->scratch_floats * 4));

    std::vector<GatherJob> jobs;
    int64_t at = 0, blocks = 0;
    for (RepackLayer &rl : P->layers) {
        const PackedConv &pc = e->convs.at(rl.name);
        for (size_t i = 0; i < rl.plan.bufs.size(); ++i) {
            BufPlan &b = rl.plan.bufs[i];
            if (b.kind == RK_CONST) continue;
            HIPCHK(hipMemcpy(maps + at, b.map.data(), b.map.size() * 4, hipMemcpyHostToDevice));
            GatherJob j;
            j.dst = pc.owned[i];
            j.map = (const int32_t *)(maps + at);
            j.src = P->scratch + rl.scratch_off;
            j.units = (int)(b.kind == RK_F32 ? b.map.size() : b.map.size() / 8);
            j.kind = b.kind;
            j.block_start = (int)blocks;
            j.pad = 0;
            jobs.push_back(j);
            blocks += (j.units + GATHER_BLOCK - 1) / GATHER_BLOCK;
            at += up256((int64_t)b.map.size() * 4);
            std::vector<int32_t>().swap(b.map);
        }
    }
    if (blocks >= ((int64_t)1 << 31)) return fail(DFFW_EINVAL, "repack plan: %lld gather workgroups", (long long)blocks);
    HIPCHK(hipMemcpy(P->jobs, jobs.data(), jobs.size() * sizeof(GatherJob), hipMemcpyHostToDevice));
    P->n_jobs = (int)jobs.size();
    P->n_blocks = (int)blocks;
    e->repack = P.release();
    return DFFW_OK;
}

}  // namespace

}  // namespace dffw

using namespace dffw;

extern "C" {

int dffw_engine_update(dffw_engine *e, const dffw_tensor *tensors, int n_tensors, void *hip_stream) {
    dffw_set_last_op_kernels("");
    if (!e) return fail(DFFW_EINVAL, "null engine");
    if (!tensors || n_tensors <= 0) return fail(DFFW_EINVAL, "no tensors given");
    std::map<std::string, const dffw_tensor *> by;
    for (int i = 0; i < n_tensors; ++i) {
        if (!tensors[i].name) return fail(DFFW_EINVAL, "tensor %d has no name", i);
        std::string nm = tensors[i].name;
        if (nm.rfind("module.", 0) == 0) nm = nm.substr(7);
        by[nm] = &tensors[i];
    }
    auto need = [&](const std::string &nm, int64_t numel, const float **p) -> int {
        auto it = by.find(nm);
        if (it == by.end()) return fail(DFFW_EMISSING, "state dict has no entry '%s'", nm.c_str());
        if (it->second->numel != numel)
            return fail(DFFW_EINVAL, "'%s' has %lld elements, expected %lld", nm.c_str(), (long long)it->second->numel, (long long)numel);
        if (!it->second->data) return fail(DFFW_EINVAL, "'%s' has null data", nm.c_str());
        if (!aligned(it->second->data, 4)) return fail(DFFW_EINVAL, "'%s' is not 4-byte aligned", nm.c_str());
        *p = it->second->data;
        return DFFW_OK;
    };

    // every parameter of every live layer, as dffw_engine_create reads them; the packed layers each one feeds (itself, or its #ref / #cur halves too)
    struct Src {
        FoldLayer f;
        std::string name;
    };
    std::vector<Src> srcs;
    const std::vector<LayerDef> &table = net_layers(e->net);
    std::map<std::string, const LayerDef *> def_of;
    for (const LayerDef &L : table) def_of[L.conv] = &L;
    for (const LayerDef &L : table) {
        if (!L.live || L.folded) continue;
        FoldLayer f;
        memset(&f, 0, sizeof f);
        int rc;
        int scin = 0;
        if (!L.shortcut.empty()) {
            const LayerDef &S = *def_of.at(L.shortcut);
            scin = S.cin;
            if ((rc = need(S.conv + ".weight", (int64_t)S.cin * S.cout, &f.sc))) return rc;
        }
        const int kvol = L.kd * L.kh * L.kw;
        if ((rc = need(L.conv + ".weight", (int64_t)L.cin * L.cout * kvol, &f.w))) return rc;
        if (L.bias && (rc = need(L.conv + ".bias", L.cout, &f.cb))) return rc;
        if (!L.bn.empty()) {
            if ((rc = need(L.bn + ".weight", L.cout, &f.g)) || (rc = need(L.bn + ".bias", L.cout, &f.b)) || (rc = need(L.bn + ".running_mean", L.cout, &f.m)) ||
                (rc = need(L.bn + ".running_var", L.cout, &f.v)))
                return rc;
        }
        f.n_w = L.cin * L.cout * kvol;
        f.n_sc = L.cout * scin;
        f.cout = L.cout;
        f.row = f.src_row = L.cin * kvol;
        f.kvol = kvol;
        f.flags = L.transposed ? FOLD_TRANSPOSED : 0;
        srcs.push_back(Src{f, L.conv});
        if (L.head_split > 0 && !L.bn.empty()) {
            // conv over [ref (C) | cur (C) | flow (2)]: two packed layers over channel slices of this weight; the ref half takes the BatchNorm scale only
            const int C = L.head_split;
            FoldLayer r = f, c = f;
            r.cb = c.cb = nullptr;
            r.row = C * kvol; r.src_off = 0; r.n_w = L.cout * r.row; r.flags |= FOLD_ZERO_SHIFT;
            c.row = (L.cin - C) * kvol; c.src_off = C * kvol; c.n_w = L.cout * c.row;
            srcs.push_back(Src{r, L.conv + "#ref"});
            srcs.push_back(Src{c, L.conv + "#cur"});
        }
    }
    if (srcs.size() != e->convs.size()) return fail(DFFW_EINVAL, "the engine holds %zu packed layers, the layer table gives %zu", e->convs.size(), srcs.size());

    HIPCHK(hipSetDevice(e->device));
    if (!e->repack) {
        const int rc = build_plan(e);
        if (rc) return rc;
    }
    const RepackPlan &P = *e->repack;
    std::map<std::string, const RepackLayer *> plan_of;
    for (const RepackLayer &rl : P.layers) plan_of[rl.name] = &rl;
    for (Src &s : srcs) {
        auto it = plan_of.find(s.name);
        if (it == plan_of.end()) return fail(DFFW_EINVAL, "the engine holds no packed layer '%s'", s.name.c_str());
        const LayerPlan &lp = it->second->plan;
        if (lp.n_w != s.f.n_w || lp.n_sc != s.f.n_sc || lp.cout != s.f.cout || lp.has_bias != (s.f.cb != nullptr))
            return fail(DFFW_EINVAL, "packed layer '%s' does not have the shape the layer table gives it", s.name.c_str());
        s.f.scratch_off = (int)it->second->scratch_off;
    }

    // from here on: launches only
    hipStream_t st = (hipStream_t)hip_stream;
    std::string names;
    FoldTable tab;
    memset(&tab, 0, sizeof tab);
    tab.scratch = P.scratch;
    auto flush = [&]() -> hipError_t {
        if (!tab.n_layers) return hipSuccess;
        const hipError_t h = launch_repack_fold(tab, st);
        names += (names.empty() ? "" : ";") + std::string(fold_kernel_name());
        tab.n_layers = tab.n_blocks = 0;
        return h;
    };
    for (const Src &s : srcs) {
        if (tab.n_layers == FOLD_LAYERS_PER_LAUNCH) HIPCHK(flush());
        FoldLayer &f = tab.layer[tab.n_layers++];
        f = s.f;
        f.block_start = tab.n_blocks;
        tab.n_blocks += std::max(1, (f.n_w + f.n_sc + FOLD_CHUNK - 1) / FOLD_CHUNK);
    }
    HIPCHK(flush());
    HIPCHK(launch_repack_gather(e->prec, P.jobs, P.n_jobs, P.n_blocks, st));
    names += std::string(";") + gather_kernel_name();
    dffw_set_last_op_kernels(names.c_str());
    return DFFW_OK;
}

int dffw_engine_repack_stats(const dffw_engine *e, int64_t out[4]) {
    if (!e || !out) return fail(DFFW_EINVAL, "null argument");
    if (!e->repack) return fail(DFFW_EINVAL, "the engine has no repack plan yet: it is built by the first dffw_engine_update");
    out[0] = e->repack->device_bytes;
    out[1] = e->repack->fold_bytes;
    out[2] = e->repack->map_bytes;
    out[3] = e->repack->buffer_bytes;
    return DFFW_OK;
}

int64_t dffw_engine_packed_bytes(const dffw_engine *e) {
    if (!e) return fail(DFFW_EINVAL, "null engine");
    int64_t n = 0;
    for (const auto &kv : e->convs)
        for (size_t b : kv.second.owned_bytes) n += (int64_t)b;
    return n;
}

int dffw_engine_packed_read(dffw_engine *e, void *host_dst, int64_t capacity, void *hip_stream) {
    if (!e || !host_dst) return fail(DFFW_EINVAL, "null argument");
    const int64_t n = dffw_engine_packed_bytes(e);
    if (capacity < n) return fail(DFFW_EINVAL, "the packed buffers are %lld bytes, the destination holds %lld", (long long)n, (long long)capacity);
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
    char *dst = (char *)host_dst;
    for (const auto &kv : e->convs) {
        const PackedConv &pc = kv.second;
        for (size_t i = 0; i < pc.owned.size(); ++i) {
            HIPCHK(hipMemcpy(dst, pc.owned[i], pc.owned_bytes[i], hipMemcpyDeviceToHost));
            dst += pc.owned_bytes[i];
        }
    }
    return DFFW_OK;
}

}  // extern "C"
