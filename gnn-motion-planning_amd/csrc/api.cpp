// api.cpp -- host side of the C ABI (include/gnnmp.h): weight manifest and packing, workspace
// carving and the kernel sequence of the explorer forward pass.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gnnmp.h"
#include "kernels.hpp"
#include "layout.hpp"

using namespace gnnmp;

namespace {

thread_local std::string g_hip_error;

int hip_fail(hipError_t e) {
    g_hip_error = hipGetErrorString(e);
    return GNNMP_ERR_HIP;
}

#define HIP_TRY(expr)                              \
    do {                                           \
        hipError_t _e = (expr);                    \
        if (_e != hipSuccess) return hip_fail(_e); \
    } while (0)

struct Entry {
    std::string name;
    int rows, cols;     // cols == 0 -> vector of `rows`
    int64_t numel() const { return (int64_t)rows * (cols ? cols : 1); }
};

// ---------------------------------------------------------------------------------------------
// explorer manifest: the 142 state_dict tensors forward() reads
// ---------------------------------------------------------------------------------------------
std::vector<Entry> explorer_manifest(const gnnmp_explorer_dims& d) {
    const int C = d.config_size, D = d.embed_size, S = d.obs_size;
    std::vector<Entry> m;
    auto lin = [&](const std::string& n, int out, int in, bool bias = true) {
        m.push_back({n + ".weight", out, in});
        if (bias) m.push_back({n + ".bias", out, 0});
    };
    auto mlp2 = [&](const std::string& n, int in) { lin(n + ".0", D, in); lin(n + ".2", D, D); };
    m.push_back({"goal_encoder", D, 0});
    mlp2("node_code", 4 * C);
    mlp2("edge_code", 2 * C);
    mlp2("obs_node_code", S);
    mlp2("obs_edge_code", S);
    mlp2("node_free_code", C);
    mlp2("edge_free_code", 2 * C);
    for (const char* side : {"node_attentions", "edge_attentions"})
        for (int b = 0; b < 3; ++b) {
            const std::string p = std::string(side) + "." + std::to_string(b);
            lin(p + ".attention.key", D, D, false);
            lin(p + ".attention.query", D, D, false);
            lin(p + ".attention.value", D, D, false);
            m.push_back({p + ".attention.layer_norm.weight", D, 0});
            m.push_back({p + ".attention.layer_norm.bias", D, 0});
            for (const char* ff : {"map_feed", "obs_feed"}) {
                lin(p + "." + ff + ".w_1", D, D);
                lin(p + "." + ff + ".w_2", D, D);
                m.push_back({p + "." + ff + ".layer_norm.weight", D, 0});
                m.push_back({p + "." + ff + ".layer_norm.bias", D, 0});
            }
        }
    lin("encoder", D, 4 * D);
    lin("process.lin_0.0", D, 5 * D);
    lin("process.lin_0.2", D, D);
    lin("process.lin_1", D, 2 * D);
    lin("decoder", D, 2 * D);
    lin("policy.0", D, 3 * D);
    lin("policy.2", D, D);
    lin("policy.4", 1, D, false);
    return m;
}

struct Blob {          // host view of the caller's concatenated weights
    std::vector<Entry> man;
    std::vector<int64_t> off;
    const float* base;
    const float* get(const std::string& n) const {
        for (size_t i = 0; i < man.size(); ++i)
            if (man[i].name == n) return base + off[i];
        return nullptr;
    }
};

bool dims_ok(const gnnmp_explorer_dims& d) {
    return d.config_size >= 1 && d.config_size <= 64 && (d.embed_size == 32 || d.embed_size == 64) &&
           d.obs_size >= 1 && d.obs_size <= 64 &&
           (d.mlp_dtype == GNNMP_F32 || d.mlp_dtype == GNNMP_BF16 || d.mlp_dtype == GNNMP_BF16X3);
}

// round-to-nearest-even fp32 -> bf16 (what v_cvt_pk_bf16_f32 does on the device)
uint16_t to_bf16(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);     // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

void pack_a_tiles_bf16(const float* w, int out_f, int ld, int col0, int n_in, float* dst_f) {
    uint16_t* dst = reinterpret_cast<uint16_t*>(dst_f);
    const int nto = out_f / 32, nti = n_in / 32;
    for (int ot = 0; ot < nto; ++ot)
        for (int it = 0; it < nti; ++it)
            for (int m = 0; m < 2; ++m)
                for (int lane = 0; lane < 64; ++lane)
                    for (int t = 0; t < 8; ++t)
                        dst[((size_t)((ot * nti + it) * 2 + m) * 64 + lane) * 8 + t] =
                            to_bf16(w[(size_t)(32 * ot + (lane & 31)) * ld + col0 + 32 * it + phi(8 * m + t, lane >> 5)]);
}

// bf16x3: every fp32 weight as three bf16 pieces w = w0 + w1 + w2 (exact for normal numbers)
void split3(float w, uint16_t (&pc)[3]) {
    float r = w;
    for (int i = 0; i < 3; ++i) {
        pc[i] = to_bf16(r);
        uint32_t u = (uint32_t)pc[i] << 16;
        float f;
        std::memcpy(&f, &u, 4);
        r -= f;
    }
}

void pack_a_tiles_bf16x3(const float* w, int out_f, int ld, int col0, int n_in, float* dst_f) {
    uint16_t* dst = reinterpret_cast<uint16_t*>(dst_f);
    const int nto = out_f / 32, nti = n_in / 32;
    for (int ot = 0; ot < nto; ++ot)
        for (int it = 0; it < nti; ++it)
            for (int m = 0; m < 2; ++m)
                for (int lane = 0; lane < 64; ++lane)
                    for (int t = 0; t < 8; ++t) {
                        uint16_t pc[3];
                        split3(w[(size_t)(32 * ot + (lane & 31)) * ld + col0 + 32 * it + phi(8 * m + t, lane >> 5)], pc);
                        for (int q = 0; q < 3; ++q)
                            dst[(((size_t)(ot * nti + it) * 3 + q) * 2 + m) * 512 + lane * 8 + t] = pc[q];
                    }
}

void pack_a_small_bf16x3(const float* w, int out_f, int ld, int col0, int n_in, float* dst_f) {
    uint16_t* dst = reinterpret_cast<uint16_t*>(dst_f);
    const int nto = out_f / 32, ks = (n_in + 15) / 16;
    for (int ot = 0; ot < nto; ++ot)
        for (int st = 0; st < ks; ++st)
            for (int lane = 0; lane < 64; ++lane)
                for (int t = 0; t < 8; ++t) {
                    const int k = 16 * st + 8 * (lane >> 5) + t;
                    uint16_t pc[3];
                    split3(k < n_in ? w[(size_t)(32 * ot + (lane & 31)) * ld + col0 + k] : 0.f, pc);
                    for (int q = 0; q < 3; ++q) dst[(((size_t)(ot * ks + st) * 3 + q) * 64 + lane) * 8 + t] = pc[q];
                }
}

void pack_a_small_bf16(const float* w, int out_f, int ld, int col0, int n_in, float* dst_f) {
    uint16_t* dst = reinterpret_cast<uint16_t*>(dst_f);
    const int nto = out_f / 32, ks = (n_in + 15) / 16;
    for (int ot = 0; ot < nto; ++ot)
        for (int st = 0; st < ks; ++st)
            for (int lane = 0; lane < 64; ++lane)
                for (int t = 0; t < 8; ++t) {
                    const int k = 16 * st + 8 * (lane >> 5) + t;
                    dst[((size_t)(ot * ks + st) * 64 + lane) * 8 + t] =
                        to_bf16(k < n_in ? w[(size_t)(32 * ot + (lane & 31)) * ld + col0 + k] : 0.f);
                }
}

std::vector<float> matvec(const float* w, int D, int ld, int col0, int n, const float* x) {
    std::vector<float> r(D);
    for (int i = 0; i < D; ++i) {
        float s = 0.f;
        for (int k = 0; k < n; ++k) s = std::fmaf(w[(size_t)i * ld + col0 + k], x[k], s);
        r[i] = s;
    }
    return r;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// exported host-only packing helpers
// ---------------------------------------------------------------------------------------------
extern "C" int64_t gnnmp_pack_a_tiles(const float* w, int out_f, int ld, int col0, int n_in, float* dst) {
    const int nto = out_f / 32, nti = n_in / 32;
    for (int ot = 0; ot < nto; ++ot)
        for (int it = 0; it < nti; ++it)
            for (int r = 0; r < 16; ++r)
                for (int lane = 0; lane < 64; ++lane)
                    dst[(size_t)(ot * nti + it) * 1024 + ((r >> 2) * 64 + lane) * 4 + (r & 3)] =
                        w[(size_t)(32 * ot + (lane & 31)) * ld + col0 + 32 * it + phi(r, lane >> 5)];
    return (int64_t)nto * nti * 1024;
}

extern "C" int64_t gnnmp_pack_a_small(const float* w, int out_f, int ld, int col0, int n_in, float* dst) {
    const int nto = out_f / 32, ks = (n_in + 1) / 2;
    for (int ot = 0; ot < nto; ++ot)
        for (int st = 0; st < ks; ++st)
            for (int lane = 0; lane < 64; ++lane) {
                const int k = 2 * st + (lane >> 5);
                dst[(size_t)(ot * ks + st) * 64 + lane] = (k < n_in) ? w[(size_t)(32 * ot + (lane & 31)) * ld + col0 + k] : 0.f;
            }
    return (int64_t)nto * ks * 64;
}

extern "C" int64_t gnnmp_pack_f64_ops(const float* w, int out_f, int ld, int col0, int n_in, int row_perm, float* dst) {
    if (!w || !dst || out_f < 16 || out_f % 16 || n_in < 1) return GNNMP_ERR_ARG;
    const int nks = (n_in + 3) / 4;
    for (int ob = 0; ob < out_f / 16; ++ob)
        for (int ks = 0; ks < nks; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int k = 4 * ks + (l >> 4), i = l & 15;
                const int row = 16 * ob + (row_perm ? 4 * (i & 3) + (i >> 2) : i);
                dst[((size_t)ob * nks + ks) * 64 + l] = k < n_in ? w[(size_t)row * ld + col0 + k] : 0.f;
            }
    return (int64_t)(out_f / 16) * nks * 64;
}

extern "C" int64_t gnnmp_pack_vec(const float* b, int n, float* dst) {
    const int nt = n / 32;
    for (int t = 0; t < nt; ++t)
        for (int h = 0; h < 2; ++h)
            for (int r = 0; r < 16; ++r) dst[(t * 2 + h) * 16 + r] = b[32 * t + phi(r, h)];
    return (int64_t)nt * 32;
}

// ---------------------------------------------------------------------------------------------
// status
// ---------------------------------------------------------------------------------------------
extern "C" const char* gnnmp_status_string(int s) {
    switch (s) {
        case GNNMP_OK: return "ok";
        case GNNMP_ERR_NULL: return "null pointer argument";
        case GNNMP_ERR_DIMS: return "unsupported or inconsistent dimensions";
        case GNNMP_ERR_WEIGHTS: return "weight blob size does not match the manifest";
        case GNNMP_ERR_WORKSPACE: return "workspace too small or misaligned";
        case GNNMP_ERR_HIP: return "HIP runtime error";
        case GNNMP_ERR_ARG: return "bad scalar argument";
        case GNNMP_ERR_CAPS: return "a caller promise was exceeded on the device (max_obstacles / max_path / max_samples / max_edges): results are wrong";
        case GNNMP_ERR_INDEX: return "edge_index holds node ids outside [0, N_g): results are wrong";
    }
    return "unknown status";
}
extern "C" const char* gnnmp_last_hip_error(void) { return g_hip_error.c_str(); }
// 2: stage list of gnnmp_explorer_profile_read (fused message passing); 3: device-side status words (gnnmp_*_status*)
extern "C" int gnnmp_abi_version(void) { return 9; }

// ---------------------------------------------------------------------------------------------
// explorer handle
// ---------------------------------------------------------------------------------------------
// optional per-stage timing with HIP events recorded on the forward's own stream
struct StageProf {
    bool on = false;
    struct Rec { int stage; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
};

struct gnnmp_explorer {
    gnnmp_explorer_dims dims;
    int device;
    float* w_dev;
    ExplorerOffsets off;
    EncBlob enc_e, enc_n;
    ObsBlob obs;
    StageProf* prof;      // mutable side state (profiling is single-threaded by contract)
    int n_cu;             // compute units of the device (persistent-kernel grid)
    int resident;         // use pre_resident_kernel when it fits (GNNMP_RESIDENT=0 disables)
    int resident_both;    // small batches: node and edge pre stages in one launch (GNNMP_PRE_BOTH=0 disables)
    int node_f64;         // node side block 0 in double precision (fp32-class modes; GNNMP_NODE_F64=0 disables, for attribution runs)
    int f64_groups;       // 64-row groups per workgroup of that role: 0 = chosen per launch (GNNMP_F64_GROUPS forces 1, 4, 8, 12 or 16)
    float* w_raw_dev;     // the caller's weight blob as given (manifest order, torch row-major): the training path's view
    std::vector<Entry> man;
    std::vector<int64_t> man_off;
    int64_t n_raw;
};

namespace {
struct StageScope {
    StageProf* p; hipStream_t st; hipEvent_t b = nullptr;
    StageScope(StageProf* p_, int stage, hipStream_t s) : p(p_ && p_->on ? p_ : nullptr), st(s) {
        if (!p) return;
        hipEvent_t a = p->get();
        b = p->get();
        (void)hipEventRecord(a, st);
        p->recs.push_back({stage, a, b});
    }
    ~StageScope() { if (p) (void)hipEventRecord(b, st); }
};
}  // namespace

extern "C" int gnnmp_explorer_manifest(const gnnmp_explorer_dims* dims, int index, char* name, size_t name_cap,
                                       int64_t* numel) {
    if (!dims) return GNNMP_ERR_NULL;
    if (!dims_ok(*dims)) return GNNMP_ERR_DIMS;
    const auto m = explorer_manifest(*dims);
    if (index < 0) return (int)m.size();
    if (index >= (int)m.size()) return GNNMP_ERR_ARG;
    if (name && name_cap) {
        std::strncpy(name, m[index].name.c_str(), name_cap - 1);
        name[name_cap - 1] = 0;
    }
    if (numel) *numel = m[index].numel();
    return GNNMP_OK;
}

namespace {

template <int D, int P>
void pack_explorer(const Blob& B, const gnnmp_explorer_dims& dm, gnnmp_explorer* h, std::vector<float>& out) {
    const int C = dm.config_size, S = dm.obs_size;
    h->enc_e = EncBlob::make(P, D, 2 * C, 2 * C);              // both edge encoders read [v_src, v_dst]
    h->enc_n = EncBlob::make(P, D, 4 * C, C);                  // node_code reads 4C numbers, node_free_code C
    h->obs = ObsBlob::make(P, D, S);
    ExplorerOffsets& o = h->off;
    int cur = 0;
    auto take = [&](int n) { const int r = cur; cur += (n + 3) & ~3; return r; };
    o.enc_e = take(h->enc_e.size);
    o.enc_n = take(h->enc_n.size);
    o.att_e = take(3 * AttBlob<D, P>::size);
    o.att_n = take(3 * AttBlob<D, P>::size);
    o.out_e = take(OutEBlob<D, P>::size);
    o.out_n = take(OutNBlob<D, P>::size);
    o.mpn = take(MpNBlob<D, P>::size);
    o.mpn_last = take(MpNBlob<D, P>::size);
    o.mpe = take(MpEBlob<D, P>::size);
    o.pol = take(PolBlob<D, P>::size);
    o.obs_e = take(h->obs.size);
    o.obs_n = take(h->obs.size);
    o.f64 = take(F64Blob::make(D, C).size);
    o.total = cur;
    out.assign(cur, 0.f);
    float* PK = out.data();
    auto W = [&](const std::string& n) { return B.get(n); };
    auto tiles = [&](const float* w, int ld, int col0, float* dst) {
        if (P == 2) pack_a_tiles_bf16x3(w, D, ld, col0, D, dst);
        else if (P == 1) pack_a_tiles_bf16(w, D, ld, col0, D, dst);
        else gnnmp_pack_a_tiles(w, D, ld, col0, D, dst);
    };
    auto small = [&](const float* w, int ld, int n_in, float* dst) {
        if (P == 2) pack_a_small_bf16x3(w, D, ld, 0, n_in, dst);
        else if (P == 1) pack_a_small_bf16(w, D, ld, 0, n_in, dst);
        else gnnmp_pack_a_small(w, D, ld, 0, n_in, dst);
    };
    auto vec = [&](const float* b, float* dst) { gnnmp_pack_vec(b, D, dst); };

    // --- encoders on raw inputs
    auto enc = [&](const EncBlob& e, float* dst, const std::string& n0, int k0, const std::string& n1, int k1) {
        small(W(n0 + ".0.weight"), k0, k0, dst + e.as0);
        vec(W(n0 + ".0.bias"), dst + e.b0);
        tiles(W(n0 + ".2.weight"), D, 0, dst + e.a0);
        vec(W(n0 + ".2.bias"), dst + e.c0);
        small(W(n1 + ".0.weight"), k1, k1, dst + e.as1);
        vec(W(n1 + ".0.bias"), dst + e.b1);
        tiles(W(n1 + ".2.weight"), D, 0, dst + e.a1);
        vec(W(n1 + ".2.bias"), dst + e.c1);
    };
    enc(h->enc_e, PK + o.enc_e, "edge_code", 2 * C, "edge_free_code", 2 * C);
    {
        // edge_code is consumed by ONE matrix only: K_e = W1d.EF + W1e.EC + b1 with EC = W2.relu(..) + c (model.py:120, :38).
        // The edge kernels therefore produce W1e.EC + b1 directly: second encoder layer F = W1e.W2, bias W1e.c + b1
        // (products in double), one d x d product per edge less.  OutEBlob::w1e / b1 stay in the layout, unused.
        const float* w1m = W("process.lin_0.0.weight");             // [d, 5d]: columns 4d.. multiply edge_code
        const float* w2 = W("edge_code.2.weight");
        const float* c2 = W("edge_code.2.bias");
        const float* b1m = W("process.lin_0.0.bias");
        std::vector<float> F((size_t)D * D), cF(D);
        for (int i = 0; i < D; ++i) {
            for (int j = 0; j < D; ++j) {
                double acc = 0.0;
                for (int k = 0; k < D; ++k) acc += (double)w1m[(size_t)i * 5 * D + 4 * D + k] * (double)w2[(size_t)k * D + j];
                F[(size_t)i * D + j] = (float)acc;
            }
            double acc = (double)b1m[i];
            for (int k = 0; k < D; ++k) acc += (double)w1m[(size_t)i * 5 * D + 4 * D + k] * (double)c2[k];
            cF[i] = (float)acc;
        }
        tiles(F.data(), D, 0, PK + o.enc_e + h->enc_e.a0);
        vec(cF.data(), PK + o.enc_e + h->enc_e.c0);
    }
    enc(h->enc_n, PK + o.enc_n, "node_code", 4 * C, "node_free_code", C);

    // --- attention blocks (map side) and obstacle side
    using A = AttBlob<D, P>;
    for (int side = 0; side < 2; ++side) {
        const std::string sname = side == 0 ? "edge_attentions" : "node_attentions";
        float* att = PK + (side == 0 ? o.att_e : o.att_n);
        float* ob = PK + (side == 0 ? o.obs_e : o.obs_n);
        const std::string oc = side == 0 ? "obs_edge_code" : "obs_node_code";
        const ObsBlob& L = h->obs;
        small(W(oc + ".0.weight"), S, S, ob + L.as0);
        vec(W(oc + ".0.bias"), ob + L.b0);
        tiles(W(oc + ".2.weight"), D, 0, ob + L.a0);
        vec(W(oc + ".2.bias"), ob + L.c0);
        for (int b = 0; b < 3; ++b) {
            const std::string p = sname + "." + std::to_string(b);
            float* a = att + (size_t)b * A::size;
            // Wqk = Wq^T Wk (see AttBlob): [d, d], Wqk[i][j] = sum_c Wq[c][i] Wk[c][j]
            std::vector<float> wqk((size_t)D * D);
            {
                const float *wq = W(p + ".attention.query.weight"), *wk = W(p + ".attention.key.weight");
                for (int i = 0; i < D; ++i)
                    for (int j = 0; j < D; ++j) {
                        double acc = 0.0;
                        for (int c2 = 0; c2 < D; ++c2) acc += (double)wq[(size_t)c2 * D + i] * (double)wk[(size_t)c2 * D + j];
                        wqk[(size_t)i * D + j] = (float)acc;
                    }
            }
            tiles(wqk.data(), D, 0, a + A::wqk);
            tiles(W(p + ".attention.value.weight"), D, 0, a + A::wv);
            if (side == 1 && b == 0) {
                // node side, block 0 in fp64 (node_f64_body): node_free_code's encoder + this block's Wqk, Wv, LayerNorm
                const F64Blob F = F64Blob::make(D, C);
                float* f = PK + o.f64;
                gnnmp_pack_f64_ops(W("node_free_code.0.weight"), D, C, 0, C, 0, f + F.w1);
                std::memcpy(f + F.b1, W("node_free_code.0.bias"), sizeof(float) * D);
                gnnmp_pack_f64_ops(W("node_free_code.2.weight"), D, D, 0, D, 0, f + F.w2);
                std::memcpy(f + F.b2, W("node_free_code.2.bias"), sizeof(float) * D);
                gnnmp_pack_f64_ops(wqk.data(), D, D, 0, D, 1, f + F.wqk);               // these two run on the f32 instruction
                gnnmp_pack_f64_ops(W(p + ".attention.value.weight"), D, D, 0, D, 1, f + F.wv);
                std::memcpy(f + F.lng, W(p + ".attention.layer_norm.weight"), sizeof(float) * D);
                std::memcpy(f + F.lnb, W(p + ".attention.layer_norm.bias"), sizeof(float) * D);
            }
            vec(W(p + ".attention.layer_norm.weight"), a + A::ln1g);
            vec(W(p + ".attention.layer_norm.bias"), a + A::ln1b);
            tiles(W(p + ".map_feed.w_1.weight"), D, 0, a + A::w1);
            vec(W(p + ".map_feed.w_1.bias"), a + A::b1);
            tiles(W(p + ".map_feed.w_2.weight"), D, 0, a + A::w2);
            vec(W(p + ".map_feed.w_2.bias"), a + A::b2);
            vec(W(p + ".map_feed.layer_norm.weight"), a + A::ln2g);
            vec(W(p + ".map_feed.layer_norm.bias"), a + A::ln2b);
            float* q = ob + L.blk0 + (size_t)b * L.blk_stride;
            tiles(wqk.data(), D, 0, q + L.wk);                       // obstacle keys are premultiplied: K' = Wqk code
            tiles(W(p + ".attention.value.weight"), D, 0, q + L.wv);
            tiles(W(p + ".obs_feed.w_1.weight"), D, 0, q + L.fw1);
            vec(W(p + ".obs_feed.w_1.bias"), q + L.fb1);
            tiles(W(p + ".obs_feed.w_2.weight"), D, 0, q + L.fw2);
            vec(W(p + ".obs_feed.w_2.bias"), q + L.fb2);
            vec(W(p + ".obs_feed.layer_norm.weight"), q + L.lng);
            vec(W(p + ".obs_feed.layer_norm.bias"), q + L.lnb);
        }
    }

    // --- message first layer W1 = [xj-xi | xj | xi | EF | EC]  (model.py:38-39)
    const float* w1 = W("process.lin_0.0.weight");
    std::vector<float> wsrc((size_t)D * D), wdst((size_t)D * D);
    for (int i = 0; i < D; ++i)
        for (int k = 0; k < D; ++k) {
            const float a = w1[(size_t)i * 5 * D + k], b = w1[(size_t)i * 5 * D + D + k], c = w1[(size_t)i * 5 * D + 2 * D + k];
            wsrc[(size_t)i * D + k] = a + b;      // multiplies x_j (source)
            wdst[(size_t)i * D + k] = c - a;      // multiplies x_i (target)
        }
    // --- policy first layer P0 = [D_s | D_s - D_t | EF]  (model.py:145)
    const float* p0 = W("policy.0.weight");
    std::vector<float> wps((size_t)D * D), wpt((size_t)D * D);
    for (int i = 0; i < D; ++i)
        for (int k = 0; k < D; ++k) {
            wps[(size_t)i * D + k] = p0[(size_t)i * 3 * D + k] + p0[(size_t)i * 3 * D + D + k];
            wpt[(size_t)i * D + k] = p0[(size_t)i * 3 * D + D + k];
        }
    {
        using L = OutEBlob<D, P>;
        float* q = PK + o.out_e;
        tiles(w1, 5 * D, 3 * D, q + L::w1d);
        tiles(w1, 5 * D, 4 * D, q + L::w1e);
        vec(W("process.lin_0.0.bias"), q + L::b1);
        tiles(p0, 3 * D, 2 * D, q + L::wpc);
        vec(W("policy.0.bias"), q + L::bp0);
    }
    const float* we = W("encoder.weight");      // [NC | NF | H0 | H]  (model.py:141)
    const float* wd = W("decoder.weight");      // [NC | H]            (model.py:143)
    const float* wl1 = W("process.lin_1.weight");   // [X | agg]       (model.py:36)
    {
        using L = OutNBlob<D, P>;
        float* q = PK + o.out_n;
        tiles(we, 4 * D, 0, q + L::we_nc);
        tiles(we, 4 * D, D, q + L::we_nf);
        vec(W("encoder.bias"), q + L::be);
        const float* ge = W("goal_encoder");
        vec(matvec(we, D, 4 * D, 2 * D, D, ge).data(), q + L::weg);
        vec(matvec(we, D, 4 * D, 3 * D, D, ge).data(), q + L::wehg);
        tiles(wsrc.data(), D, 0, q + L::wsrc);
        tiles(wdst.data(), D, 0, q + L::wdst);
        tiles(wd, 2 * D, 0, q + L::wd_nc);
        vec(W("decoder.bias"), q + L::bd);
    }
    for (int last = 0; last < 2; ++last) {
        using L = MpNBlob<D, P>;
        float* q = PK + (last ? o.mpn_last : o.mpn);
        tiles(wl1, 2 * D, 0, q + L::wlx);
        tiles(wl1, 2 * D, D, q + L::wla);
        vec(W("process.lin_1.bias"), q + L::bl);
        if (!last) {
            tiles(we, 4 * D, 3 * D, q + L::m1);
            tiles(wsrc.data(), D, 0, q + L::m2);
            tiles(wdst.data(), D, 0, q + L::m3);
        } else {
            tiles(wd, 2 * D, D, q + L::m1);
            tiles(wps.data(), D, 0, q + L::m2);
            tiles(wpt.data(), D, 0, q + L::m3);
        }
    }
    {
        using L = MpEBlob<D, P>;
        float* q = PK + o.mpe;
        tiles(W("process.lin_0.2.weight"), D, 0, q + L::w2);
        vec(W("process.lin_0.2.bias"), q + L::b2);
    }
    {
        using L = PolBlob<D, P>;
        float* q = PK + o.pol;
        tiles(W("policy.2.weight"), D, 0, q + L::w2);
        vec(W("policy.2.bias"), q + L::b2);
        vec(W("policy.4.weight"), q + L::w3);
    }
}

}  // namespace

extern "C" int gnnmp_explorer_create(gnnmp_explorer** out, const gnnmp_explorer_dims* dims, const float* weights_host,
                                     size_t n_floats, int device) {
    if (!out || !dims || !weights_host) return GNNMP_ERR_NULL;
    if (!dims_ok(*dims)) return GNNMP_ERR_DIMS;
    Blob B;
    B.man = explorer_manifest(*dims);
    B.base = weights_host;
    int64_t tot = 0;
    for (auto& e : B.man) { B.off.push_back(tot); tot += e.numel(); }
    if ((int64_t)n_floats != tot) return GNNMP_ERR_WEIGHTS;
    gnnmp_explorer* h = new gnnmp_explorer();
    h->dims = *dims;
    h->device = device;
    h->w_dev = nullptr;
    h->w_raw_dev = nullptr;
    h->man = B.man; h->man_off = B.off; h->n_raw = tot;
    h->prof = new StageProf();
    std::vector<float> packed;
    const int P = dims->mlp_dtype;
    if (dims->embed_size == 32) {
        if (P == 2) pack_explorer<32, 2>(B, *dims, h, packed);
        else if (P == 1) pack_explorer<32, 1>(B, *dims, h, packed);
        else pack_explorer<32, 0>(B, *dims, h, packed);
    } else {
        if (P == 2) pack_explorer<64, 2>(B, *dims, h, packed);
        else if (P == 1) pack_explorer<64, 1>(B, *dims, h, packed);
        else pack_explorer<64, 0>(B, *dims, h, packed);
    }
    // the handle lives on `device`; the caller's current device is restored before returning
    int prev_dev = -1;
    (void)hipGetDevice(&prev_dev);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) {
        int ncu = 0;
        e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device);
        h->n_cu = (ncu > 0 ? ncu : 256) & ~7;
        if (h->n_cu < 8) h->n_cu = 8;
        const char* env = std::getenv("GNNMP_RESIDENT");
        h->resident = !(env && env[0] == '0');
        const char* env2 = std::getenv("GNNMP_PRE_BOTH");
        h->resident_both = !(env2 && env2[0] == '0');
        const char* env3 = std::getenv("GNNMP_NODE_F64");
        h->node_f64 = !(env3 && env3[0] == '0');
        const char* env4 = std::getenv("GNNMP_F64_GROUPS");
        const int fg = env4 ? std::atoi(env4) : 0;
        h->f64_groups = (fg == 1 || (fg >= 4 && fg <= 16 && fg % 4 == 0)) ? fg : 0;
    }
    if (e == hipSuccess) e = hipMalloc((void**)&h->w_dev, packed.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->w_dev, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&h->w_raw_dev, (size_t)tot * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->w_raw_dev, weights_host, (size_t)tot * sizeof(float), hipMemcpyHostToDevice);
    if (prev_dev >= 0 && prev_dev != device) (void)hipSetDevice(prev_dev);
    if (e != hipSuccess) {
        if (h->w_dev) (void)hipFree(h->w_dev);
        if (h->w_raw_dev) (void)hipFree(h->w_raw_dev);
        delete h->prof;
        delete h;
        return hip_fail(e);
    }
    *out = h;
    return GNNMP_OK;
}

extern "C" int gnnmp_explorer_destroy(gnnmp_explorer* h) {
    if (!h) return GNNMP_ERR_NULL;
    if (h->w_dev) (void)hipFree(h->w_dev);
    if (h->w_raw_dev) (void)hipFree(h->w_raw_dev);
    if (h->prof) {
        for (auto& r : h->prof->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
        for (auto e : h->prof->pool) (void)hipEventDestroy(e);
        delete h->prof;
    }
    delete h;
    return GNNMP_OK;
}

extern "C" int gnnmp_explorer_profile(gnnmp_explorer* h, int enable) {
    if (!h) return GNNMP_ERR_NULL;
    h->prof->on = enable != 0;
    // create the events up front so that no hipEventCreate lands inside a timed region
    if (h->prof->on)
        while (h->prof->pool.size() < 2048) {
            hipEvent_t e = nullptr;
            HIP_TRY(hipEventCreate(&e));
            h->prof->pool.push_back(e);
        }
    return GNNMP_OK;
}

extern "C" int gnnmp_explorer_profile_read(gnnmp_explorer* h, double* ms_sum, int64_t* launches) {
    if (!h || !ms_sum || !launches) return GNNMP_ERR_NULL;
    for (int i = 0; i < GNNMP_N_STAGES; ++i) { ms_sum[i] = 0.0; launches[i] = 0; }
    for (auto& r : h->prof->recs) {
        HIP_TRY(hipEventSynchronize(r.b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        ms_sum[r.stage] += ms;
        launches[r.stage] += 1;
        h->prof->pool.push_back(r.a);
        h->prof->pool.push_back(r.b);
    }
    h->prof->recs.clear();
    return GNNMP_OK;
}

// ---------------------------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------------------------
namespace {

struct Carve {
    // sizes
    int G, Npad, Epad, ot_max, kv_stride, D;
    // offsets in bytes
    size_t node_ptr_pad, edge_ptr_pad, goal_node, dense_ptr, in_ptrs, prep_hist, gstat;
    size_t zero_beg, deg, cursor, zero_end;
    size_t ff_beg, ntile_graph, etile_graph, csr, ff_end, tile_meta, rec32, blk_span;
    size_t row_beg;
    size_t XI, X, A, A2, B, DN, H, Ke, PE, kv_e, kv_n, M0;
    size_t total;
};

int round_up_i(int x, int m) { return (x + m - 1) / m * m; }

// by embed size and precision alone: the geometry test hook carves without a handle
bool carve(int D, int mlp_dtype, const gnnmp_batch* b, Carve& c) {
    if (b->n_graphs < 1 || b->total_nodes < 0 || b->total_edges < 0 || b->total_obstacles < 0 || b->max_obstacles < 0)
        return false;
    const int NT = D / 32;
    c.D = D;
    c.G = b->n_graphs;
    const long long np = (long long)b->total_nodes + (long long)c.G * (kPad - 1);
    const long long ep = (long long)b->total_edges + (long long)c.G * (kPad - 1);
    if (np > 0x3fffffff || ep > 0x3fffffff) return false;
    c.Npad = round_up_i((int)np, kPad);
    c.Epad = round_up_i((int)ep, kPad);
    c.ot_max = (b->max_obstacles + 31) / 32;
    if (c.ot_max < 1) c.ot_max = 1;
    c.kv_stride = 2 * c.ot_max * NT * tile_unit(mlp_dtype);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    c.node_ptr_pad = take(sizeof(int) * (c.G + 1));
    c.edge_ptr_pad = take(sizeof(int) * (c.G + 1));
    c.goal_node = take(sizeof(int) * c.G);
    c.dense_ptr = take(sizeof(long long) * (c.G + 1));
    c.in_ptrs = take(sizeof(int) * 6);          // prefix arrays of a single graph given by its totals (NULL prefix pointers)
    c.gstat = take(sizeof(int) * kGstatStride * (size_t)c.G);      // device-side status of the forward (gnnmp_explorer_status)
    c.zero_beg = o;
    c.deg = take(sizeof(int) * c.Npad);
    c.zero_end = o;
    c.cursor = take(sizeof(int) * (size_t)(b->total_edges > 0 ? b->total_edges : 1));   // per-edge rank in its segment
    c.ff_beg = o;
    c.ntile_graph = take(sizeof(int) * (c.Npad / 32));
    c.etile_graph = take(sizeof(int) * (c.Epad / 32));
    c.tile_meta = take(sizeof(int) * (c.Epad / 32));            // -1 = tile beyond the last graph
    c.csr = take(sizeof(int) * 4 * (size_t)c.Epad);
    c.ff_end = o;
    c.rec32 = take(sizeof(int) * (size_t)c.Epad);
    c.blk_span = take(sizeof(int) * 2 * (size_t)(c.Npad / kPad));
    c.row_beg = take(sizeof(int) * c.Npad);
    {   // per-part target histograms + first slots of the prep stage's two-launch form (large graphs only)
        const int parts = prep_parts(c.G, b->total_edges);
        c.prep_hist = take(parts > 1 ? sizeof(int) * 2 * (size_t)parts * c.Npad : 0);
    }
    const size_t nrow = sizeof(float) * (size_t)c.Npad * D, erow = sizeof(float) * (size_t)c.Epad * D;
    c.XI = take(nrow); c.X = take(nrow); c.A = take(nrow); c.A2 = take(nrow); c.B = take(nrow); c.DN = take(nrow);
    c.H = take(nrow);
    c.M0 = take(mlp_dtype == GNNMP_BF16 ? 0 : nrow);      // node_f64_body -> node pre kernel (fp32-class modes)
    c.Ke = take(erow); c.PE = take(erow);
    c.kv_e = take(sizeof(float) * (size_t)c.G * 3 * c.kv_stride);
    c.kv_n = take(sizeof(float) * (size_t)c.G * 3 * c.kv_stride);
    c.total = o;
    return true;
}
bool carve(const gnnmp_explorer* h, const gnnmp_batch* b, Carve& c) { return carve(h->dims.embed_size, h->dims.mlp_dtype, b, c); }

template <class T>
T* at(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }

// LDS plan of pre_kernel: weight region + K/V chunk region
struct PrePlan { int waves, ot_chunk, wregion; size_t lds_bytes; };

// blob sizes by (d, precision): T = (d/32)^2 * tile_unit(P), V = d
int out_e_size(int D, int P) { return 3 * tile_floats(D, P) + 2 * vec_floats(D); }
int out_n_size(int D, int P) { return 5 * tile_floats(D, P) + 4 * vec_floats(D); }
int att_staged(int D, int P) { return 4 * tile_floats(D, P); }

PrePlan plan_pre(int D, int P, int ot_max, int enc_size, int out_size, bool use_obs) {
    const int NT = D / 32;
    const int att = att_staged(D, P);
    int wr = enc_size > out_size ? enc_size : out_size;
    if (use_obs && att > wr) wr = att;
    wr = ((wr + 3) & ~3) + 32;                            // + the tail mask of the graph (explorer_kernels.hip kTailMask)
    PrePlan p;
    p.wregion = wr;
    p.waves = (D == 32) ? 4 : 8;
    const size_t per_tile = (size_t)2 * NT * tile_unit(P) * sizeof(float);
    p.ot_chunk = 1;
    if (use_obs) {
        // prefer the highest workgroups-per-CU residency that still keeps a graph's whole K/V resident
        const size_t limit = 163840, wbytes = (size_t)wr * sizeof(float);
        for (int target = (D == 32 ? 3 : 1); target >= 1; --target) {
            const size_t budget = (limit / target) & ~(size_t)1023;
            if (budget < wbytes + per_tile) continue;
            int ch = (int)((budget - wbytes) / per_tile);
            if (ch > ot_max) ch = ot_max;
            p.ot_chunk = ch;
            if (ch >= ot_max) break;
        }
    }
    p.lds_bytes = (size_t)wr * sizeof(float) + (use_obs ? (size_t)p.ot_chunk * per_tile : 0);
    return p;
}

}  // namespace

extern "C" int gnnmp_explorer_workspace_bytes(const gnnmp_explorer* h, const gnnmp_batch* shape, size_t* bytes) {
    if (!h || !shape || !bytes) return GNNMP_ERR_NULL;
    Carve c;
    if (!carve(h, shape, c)) return GNNMP_ERR_ARG;
    *bytes = c.total;
    return GNNMP_OK;
}

namespace {
int forward_impl(const gnnmp_explorer* h, const gnnmp_batch* b, int loop, int use_obstacles, float* edge_scores, float* dense,
                 void* ws, size_t ws_bytes, void* hip_stream, float* om_nodes, float* om_edges, bool pre_only, int32_t* status_out = nullptr);
}
extern "C" int gnnmp_explorer_forward(const gnnmp_explorer* h, const gnnmp_batch* b, int loop, int use_obstacles,
                                      float* edge_scores, float* dense, void* ws, size_t ws_bytes, void* hip_stream) {
    return forward_impl(h, b, loop, use_obstacles, edge_scores, dense, ws, ws_bytes, hip_stream, nullptr, nullptr, false);
}
extern "C" int gnnmp_explorer_forward_ex(const gnnmp_explorer* h, const gnnmp_batch* b, int loop, int use_obstacles,
                                         float* edge_scores, float* dense, void* ws, size_t ws_bytes, void* hip_stream,
                                         int32_t* status_out) {
    return forward_impl(h, b, loop, use_obstacles, edge_scores, dense, ws, ws_bytes, hip_stream, nullptr, nullptr, false, status_out);
}
extern "C" int gnnmp_explorer_status_words(const gnnmp_batch* shape, size_t* n_words) {
    if (!shape || !n_words) return GNNMP_ERR_NULL;
    if (shape->n_graphs < 1) return GNNMP_ERR_ARG;
    *n_words = (size_t)kGstatStride * (size_t)shape->n_graphs;
    return GNNMP_OK;
}

namespace gnnmp { hipError_t launch_status_copy(const int* src, int* dst_host_mapped, int n, hipStream_t st); }
extern "C" int gnnmp_status_copy(const int32_t* src_device, int32_t* dst_host_mapped, int32_t n_words, void* hip_stream) {
    if (!src_device || !dst_host_mapped) return GNNMP_ERR_NULL;
    if (n_words < 0) return GNNMP_ERR_ARG;
    HIP_TRY(gnnmp::launch_status_copy(src_device, dst_host_mapped, n_words, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_explorer_status_region(const gnnmp_explorer* h, const gnnmp_batch* shape, size_t* offset, size_t* bytes) {
    if (!h || !shape || !offset || !bytes) return GNNMP_ERR_NULL;
    Carve c;
    if (!carve(h, shape, c)) return GNNMP_ERR_ARG;
    *offset = c.gstat;
    *bytes = sizeof(int) * kGstatStride * (size_t)c.G;
    return GNNMP_OK;
}

extern "C" int gnnmp_explorer_status_decode(const int32_t* words_host, int n_graphs, int32_t* first_graph) {
    if (!words_host || n_graphs < 0) return GNNMP_ERR_NULL;
    int caps = -1, ids = -1;
    for (int g = 0; g < n_graphs; ++g) {
        if (caps < 0 && (words_host[kGstatStride * g] & 1)) caps = g;
        for (int k = 1; k < kGstatStride && ids < 0; ++k)
            if (words_host[kGstatStride * g + k] & 2) ids = g;
    }
    if (ids >= 0) { if (first_graph) *first_graph = ids; return GNNMP_ERR_INDEX; }
    if (caps >= 0) { if (first_graph) *first_graph = caps; return GNNMP_ERR_CAPS; }
    if (first_graph) *first_graph = -1;
    return GNNMP_OK;
}

extern "C" int gnnmp_explorer_status(const gnnmp_explorer* h, const gnnmp_batch* shape, const void* ws, size_t ws_bytes,
                                     void* hip_stream, int32_t* first_graph) {
    if (!h || !shape || !ws) return GNNMP_ERR_NULL;
    Carve c;
    if (!carve(h, shape, c)) return GNNMP_ERR_ARG;
    if (ws_bytes < c.total) return GNNMP_ERR_WORKSPACE;
    std::vector<int32_t> host((size_t)kGstatStride * c.G);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipMemcpyAsync(host.data(), static_cast<const char*>(ws) + c.gstat, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return gnnmp_explorer_status_decode(host.data(), c.G, first_graph);
}

namespace {
// PrepParams of a batch over its carved workspace: the one place that fills them (the forward and the geometry test hook).
// implicit: ONE graph given by its totals, the prefix arrays are written into the workspace by the prep stage itself.
PrepParams prep_params(const Carve& c, const gnnmp_batch* b, int C, void* ws, bool implicit, int obs_cap, int* gstat) {
    PrepParams q{};
    q.G = c.G; q.E = b->total_edges; q.C = C;
    q.edge_index = reinterpret_cast<const long long*>(b->edge_index);
    q.single_out = implicit ? at<int>(ws, c.in_ptrs) : nullptr;
    q.single_n = b->total_nodes; q.single_e = b->total_edges; q.single_o = b->total_obstacles;
    q.node_ptr = implicit ? at<int>(ws, c.in_ptrs) : b->node_ptr;
    q.edge_ptr = implicit ? at<int>(ws, c.in_ptrs) + 2 : b->edge_ptr;
    q.v = b->v; q.goal = b->goal;
    q.node_ptr_pad = at<int>(ws, c.node_ptr_pad); q.edge_ptr_pad = at<int>(ws, c.edge_ptr_pad);
    q.dense_ptr = at<long long>(ws, c.dense_ptr);
    q.deg = at<int>(ws, c.deg); q.cursor = at<int>(ws, c.cursor); q.row_beg = at<int>(ws, c.row_beg);
    q.ntile_graph = at<int>(ws, c.ntile_graph); q.etile_graph = at<int>(ws, c.etile_graph);
    q.csr = at<int4>(ws, c.csr);
    q.goal_node = at<int>(ws, c.goal_node);
    q.tile_meta = at<int>(ws, c.tile_meta); q.n_etiles = c.Epad / 32;
    q.blk_span = at<int2>(ws, c.blk_span);
    q.obs_ptr = implicit ? nullptr : b->obs_ptr;
    q.obs_cap = obs_cap;
    q.gstat = gstat;
    return q;
}

// om_nodes / om_edges: optional [Npad, d] / [Epad, d] outputs of the attention stacks (training path); pre_only: stop
// after the pre kernels (CSR, goal node, NF / EF are what the training path needs)
int forward_impl(const gnnmp_explorer* h, const gnnmp_batch* b, int loop, int use_obstacles, float* edge_scores, float* dense,
                 void* ws, size_t ws_bytes, void* hip_stream, float* om_nodes, float* om_edges, bool pre_only, int32_t* status_out) {
    if (!h || !b || !ws) return GNNMP_ERR_NULL;
    if (!b->v || !b->goal) return GNNMP_ERR_NULL;
    // ONE graph may be given by its totals alone (all three prefix pointers NULL): the reference's call (model.py:115)
    // has no prefix arrays, and building them on the device costs the caller three host-to-device copies per call
    const bool implicit = !b->node_ptr && !b->edge_ptr && !b->obs_ptr;
    if (implicit ? b->n_graphs != 1 : (!b->node_ptr || !b->edge_ptr || !b->obs_ptr)) return GNNMP_ERR_NULL;
    if (b->total_edges > 0 && (!b->edge_index || (!edge_scores && !pre_only))) return GNNMP_ERR_NULL;
    if (use_obstacles && b->total_obstacles > 0 && !b->obstacles) return GNNMP_ERR_NULL;
    if (loop < 1) return GNNMP_ERR_ARG;                    // model.py:139-145: decode unbound for loop = 0
    Carve c;
    if (!carve(h, b, c)) return GNNMP_ERR_ARG;
    if (ws_bytes < c.total || (reinterpret_cast<uintptr_t>(ws) & 255)) return GNNMP_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int D = h->dims.embed_size, C = h->dims.config_size, P = h->dims.mlp_dtype;
    const float* W = h->w_dev;

    StageProf* prof = h->prof;
    PrepParams q;
    const int* node_ptr = implicit ? at<int>(ws, c.in_ptrs) : b->node_ptr;
    const int* edge_ptr = implicit ? at<int>(ws, c.in_ptrs) + 2 : b->edge_ptr;
    const int* obs_ptr = implicit ? at<int>(ws, c.in_ptrs) + 4 : b->obs_ptr;
    {
    StageScope sc(prof, GNNMP_STAGE_PREP, st);
    // the status words of this forward: the workspace region (read back by gnnmp_explorer_status), or -- gnnmp_explorer_forward_ex --
    // memory of the caller's that the device can write (pinned host memory: no copy behind the forward, the words simply arrive)
    q = prep_params(c, b, C, ws, implicit, use_obstacles ? 32 * c.ot_max : 0x7fffffff,
                    status_out ? reinterpret_cast<int*>(status_out) : at<int>(ws, c.gstat));
    HIP_TRY(launch_prep(q, c.Npad, c.Epad, at<int>(ws, c.prep_hist), st));
    // zero-fill of policy_output (model.py:148); sum_g N_g^2 is read from dense_ptr[G] on the device
    if (dense) HIP_TRY(launch_zero_dense(dense, q.dense_ptr + c.G, st));
    // training path: CSR slots in a timing-independent order (the gradients sum over slots)
    if (pre_only) HIP_TRY(t_sort_csr(c.Npad, q.csr, q.row_beg, q.deg, st));
    }

    const bool use_obs = use_obstacles != 0;
    bool use_m0 = false;
    if (use_obs) {
        ObsParams op;
        op.obstacles = b->obstacles; op.obs_ptr = obs_ptr; op.S = h->dims.obs_size;
        op.w[0] = W + h->off.obs_n; op.w[1] = W + h->off.obs_e;
        op.blob = h->obs;
        op.kv[0] = at<float>(ws, c.kv_n); op.kv[1] = at<float>(ws, c.kv_e);
        op.kv_stride = c.kv_stride; op.ot_max = c.ot_max;
        NodeF64Params nq;
        nq.v = b->v; nq.C = C; nq.node_ptr = node_ptr; nq.node_ptr_pad = q.node_ptr_pad; nq.ntile_graph = q.ntile_graph;
        nq.w = W + h->off.f64; nq.blob = F64Blob::make(D, C);
        nq.m0 = at<float>(ws, c.M0);
        nq.n_rows = c.Npad;
        const bool f64_role = P != GNNMP_BF16 && h->node_f64;
        nq.groups = c.Npad / 64 > 2 * h->n_cu ? 4 : 1;                          // kPad = 256 rows = 4 groups
        if (nq.groups == 4 && f64_role) {
            // More 256-row blocks than resident workgroups: a workgroup takes m blocks in a row when that costs no extra round --
            // rounds(m) * m block times, the larger m on a tie: it builds the obstacle operands once per graph it meets instead of
            // once per block.  Blocks in use from the caller's totals (exact for graphs of one size; the prefix arrays are on the
            // device); a workgroup whose blocks belong to different graphs rebuilds where the graph changes, so any m is correct.
            const int slots = obs_f64_slots(D, P, op, nq);
            const long long per_graph = ((long long)b->total_nodes / c.G + kPad - 1) / kPad;
            const long long blocks = per_graph * c.G;
            long long best = 0;
            for (int m = 1; m <= 4 && slots > 0; m *= 2) {
                const long long wgs = (blocks + m - 1) / m, cost = (wgs + slots - 1) / slots * m;
                if (m == 1 || cost <= best) { best = cost; nq.groups = 4 * m; }
            }
        }
        if (h->f64_groups) nq.groups = h->f64_groups;
        {
            static const char* ord = std::getenv("GNNMP_F64_FIRST");
            // measured: cfg 2 (d = 32, 1024 double-precision workgroups = two rounds) 0.145 -> 0.139 ms with them first;
            // kuka7 fp32 (d = 64, 512 = one round) 0.153 -> 0.162 ms, so d = 64 keeps the obstacle workgroups in front
            nq.f64_first = ord ? (ord[0] != '0') : (nq.groups > 1 && D == 32);
        }
        nq.n_wg = f64_role ? (c.Npad + 64 * nq.groups - 1) / (64 * nq.groups) : 0;
        use_m0 = nq.n_wg > 0;
        StageScope sc(prof, GNNMP_STAGE_OBS, st);
        HIP_TRY(launch_obs(D, P, op, nq, c.G, st));
    }

    PreParams pp[2];
    PrePlan plan[2];
    size_t res_lds[2] = {0, 0};                            // LDS bytes of the resident variant, 0 = not applicable
    const size_t res_bytes = ((size_t)3 * (att_staged(D, P) + 6 * vec_floats(D)) + (size_t)3 * c.kv_stride) * sizeof(float) + 64 + 128;   // + tile counter, tail mask
    const bool resident_ok = ((D == 32 && P == 0) || P == 1) && use_obs && res_bytes <= 163840 && h->resident;
    for (int edge = 0; edge < 2; ++edge) {
        PreParams& p = pp[edge];
        p.v = b->v; p.goal = b->goal; p.C = C;
        p.node_ptr = node_ptr; p.node_ptr_pad = q.node_ptr_pad;
        p.tile_graph = edge ? q.etile_graph : q.ntile_graph;
        p.csr = q.csr;
        p.rec32 = at<int>(ws, c.rec32);
        p.obs_ptr = obs_ptr; p.goal_node = q.goal_node;
        p.enc = W + (edge ? h->off.enc_e : h->off.enc_n);
        p.encb = edge ? h->enc_e : h->enc_n;
        p.att = W + (edge ? h->off.att_e : h->off.att_n);
        p.out = W + (edge ? h->off.out_e : h->off.out_n);
        p.out_size = edge ? out_e_size(D, P) : out_n_size(D, P);
        p.kv = at<float>(ws, edge ? c.kv_e : c.kv_n);
        p.kv_stride = c.kv_stride; p.ot_max = c.ot_max;
        plan[edge] = plan_pre(D, P, c.ot_max, p.encb.size, p.out_size, use_obs);
        p.ot_chunk = plan[edge].ot_chunk; p.wregion = plan[edge].wregion; p.use_obstacles = use_obs ? 1 : 0;
        p.om = edge ? om_edges : om_nodes;
        p.m0 = (!edge && use_m0) ? at<float>(ws, c.M0) : nullptr;
        if (edge) { p.o0 = at<float>(ws, c.Ke); p.o1 = at<float>(ws, c.PE); p.o2 = p.o3 = p.o4 = nullptr; }
        else {
            p.o0 = at<float>(ws, c.XI); p.o1 = at<float>(ws, c.X); p.o2 = at<float>(ws, c.A);
            p.o3 = at<float>(ws, c.B); p.o4 = at<float>(ws, c.DN);
        }
        // resident variant: all three blocks' weights + the graph's K/V for all three blocks in LDS
        p.ptr_pad_total = edge ? q.edge_ptr_pad : q.node_ptr_pad;
        p.tile_meta = q.tile_meta;
        p.G = c.G;
        p.out_in_lds = 0;
        if (resident_ok) {
            res_lds[edge] = res_bytes;
            if (res_bytes + (size_t)p.out_size * sizeof(float) <= 163840) {      // the epilogue weights fit as well
                p.out_in_lds = 1;
                res_lds[edge] += (size_t)p.out_size * sizeof(float);
            }
        }
    }
    // small batches: both stages in one launch, side by side (see pre_resident_both_kernel); `share` 32-row tiles per
    // 12-wave workgroup, as few as keep all workgroups of both roles resident at once
    bool both_done = false;
    if (resident_ok && D == 32 && b->total_edges > 0 && h->resident_both) {
        const int nt = c.Npad / 32, et = c.Epad / 32;
        for (int share = 1; share <= 12 && !both_done; ++share) {
            const int nb = ((nt + share - 1) / share + 7) & ~7, eb = ((et + share - 1) / share + 7) & ~7;
            if (nb + eb > h->n_cu) continue;
            StageScope sc(prof, GNNMP_STAGE_EDGE_PRE, st);
            HIP_TRY(launch_pre_resident_both(D, P, pp[0], pp[1], res_lds[0] > res_lds[1] ? res_lds[0] : res_lds[1], nb, eb, st));
            both_done = true;
        }
    }
    for (int edge = 0; edge < 2 && !both_done; ++edge) {
        if (edge && b->total_edges == 0) continue;
        StageScope sc(prof, edge ? GNNMP_STAGE_EDGE_PRE : GNNMP_STAGE_NODE_PRE, st);
        if (res_lds[edge]) HIP_TRY(launch_pre_resident(D, P, edge != 0, pp[edge], res_lds[edge], h->n_cu, st));
        else HIP_TRY(launch_pre(D, P, edge != 0, plan[edge].waves, pp[edge], (edge ? c.Epad : c.Npad) / 32, plan[edge].lds_bytes, st));
    }

    if (pre_only) return GNNMP_OK;

    // message passing: one fused launch per iteration (edge phase + node phase per 32-node tile); the gathered A rows
    // ping-pong between two buffers because other tiles still read this iteration's A while a tile writes the next one
    float* Abuf[2] = {at<float>(ws, c.A), at<float>(ws, c.A2)};
    int cur = 0;
    for (int it = 0; it < loop; ++it) {
        const bool last = (it == loop - 1);
        MpFusedParams f;
        f.rec32 = at<int>(ws, c.rec32); f.row_beg = q.row_beg; f.deg = q.deg; f.ntile_graph = q.ntile_graph; f.node_ptr_pad = q.node_ptr_pad;
        f.A = Abuf[cur]; f.B = at<float>(ws, c.B); f.Ke = at<float>(ws, c.Ke);
        f.X = at<float>(ws, c.X); f.R = at<float>(ws, last ? c.DN : c.XI);
        f.we = W + h->off.mpe; f.wn = W + (last ? h->off.mpn_last : h->off.mpn);
        f.wn_std = W + h->off.mpn; f.last = last ? 1 : 0;
        f.Hout = at<float>(ws, c.H); f.Xout = at<float>(ws, c.X); f.Aout = Abuf[cur ^ 1]; f.Bout = at<float>(ws, c.B);
        f.n_tiles = c.Npad / 32;
        f.tpw = 1;
        f.order = 0;
        f.blk_span = q.blk_span;
        f.trace = nullptr;
        f.G = c.G;
        f.store_h = last ? 1 : 0;
        StageScope sc(prof, GNNMP_STAGE_MP, st);
        HIP_TRY(launch_mp_fused(D, P, f, st));
        cur ^= 1;
    }

    if (b->total_edges > 0) {
        PolicyParams p;
        p.csr = q.csr; p.etile_graph = q.etile_graph;
        p.node_ptr = node_ptr; p.node_ptr_pad = q.node_ptr_pad; p.dense_ptr = q.dense_ptr;
        p.PS = Abuf[cur]; p.PT = at<float>(ws, c.B); p.PE = at<float>(ws, c.PE);
        p.w = W + h->off.pol;
        p.scores = edge_scores; p.dense = dense;
        p.n_tiles = c.Epad / 32;
        StageScope sc(prof, GNNMP_STAGE_POLICY, st);
        HIP_TRY(launch_policy(D, P, p, st));
    }
    return GNNMP_OK;
}
}  // namespace

extern "C" int gnnmp_explorer_debug_tap(const gnnmp_explorer* h, const gnnmp_batch* b, int which, float* dst, void* ws,
                                        size_t ws_bytes, void* hip_stream) {
    if (!h || !b || !dst || !ws) return GNNMP_ERR_NULL;
    Carve c;
    if (!carve(h, b, c)) return GNNMP_ERR_ARG;
    if (ws_bytes < c.total) return GNNMP_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int D = h->dims.embed_size;
    size_t src;
    switch (which) {
        case 0: src = c.XI; break;
        case 1: src = c.H; break;
        case 2:
            if (h->dims.mlp_dtype == GNNMP_BF16) return GNNMP_ERR_DIMS;      // X rows are stored in bf16 in that mode
            src = c.X; break;
        case 3:
            HIP_TRY(launch_goal_tap(c.G, at<int>(ws, c.goal_node), at<int>(ws, c.node_ptr_pad), dst, st));
            return GNNMP_OK;
        case 4:
            if (h->dims.mlp_dtype == GNNMP_BF16 || !h->node_f64) return GNNMP_ERR_DIMS;      // the fp64 node role did not run
            src = c.M0; break;
        default: return GNNMP_ERR_ARG;
    }
    HIP_TRY(launch_unpad_rows(c.G, b->total_nodes, D, b->node_ptr ? b->node_ptr : at<int>(ws, c.in_ptrs), at<int>(ws, c.node_ptr_pad),
                              at<float>(ws, src), dst, st));
    return GNNMP_OK;
}

// =============================================================================================
// smoother
// =============================================================================================
namespace {

std::vector<Entry> smoother_manifest(const gnnmp_smoother_dims& d) {
    const int C = d.config_size, D = d.embed_size;
    std::vector<Entry> m;
    auto lin = [&](const std::string& n, int out, int in) {
        m.push_back({n + ".weight", out, in});
        m.push_back({n + ".bias", out, 0});
    };
    lin("node_code.0", D, C + 3);
    m.push_back({"node_code.1.weight", D, 0});
    m.push_back({"node_code.1.bias", D, 0});
    m.push_back({"node_code.1.running_mean", D, 0});
    m.push_back({"node_code.1.running_var", D, 0});
    lin("node_code.3", D, D);
    lin("process.lin_0.0", D, 3 * D);
    lin("process.lin_0.2", D, D);
    lin("process.lin_1.0", D, D);
    lin("process.lin_1.2", D, D);
    lin("smooth_node", C, D);
    return m;
}

bool sm_dims_ok(const gnnmp_smoother_dims& d) {
    return d.config_size >= 1 && d.config_size <= 29 && (d.embed_size == 32 || d.embed_size == 64 || d.embed_size == 128) &&
           d.scale > 0.f && (d.mlp_dtype == GNNMP_F32 || d.mlp_dtype == GNNMP_BF16);
}

}  // namespace

struct gnnmp_smoother {
    gnnmp_smoother_dims dims;
    int device;
    float* w_dev;
    SmLayout L;
    float* w_raw_dev;     // the caller's weight blob as given (training path)
    std::vector<Entry> man;
    std::vector<int64_t> man_off;
    int64_t n_raw;
};

extern "C" int gnnmp_smoother_manifest(const gnnmp_smoother_dims* dims, int index, char* name, size_t name_cap,
                                       int64_t* numel) {
    if (!dims) return GNNMP_ERR_NULL;
    if (!sm_dims_ok(*dims)) return GNNMP_ERR_DIMS;
    const auto m = smoother_manifest(*dims);
    if (index < 0) return (int)m.size();
    if (index >= (int)m.size()) return GNNMP_ERR_ARG;
    if (name && name_cap) {
        std::strncpy(name, m[index].name.c_str(), name_cap - 1);
        name[name_cap - 1] = 0;
    }
    if (numel) *numel = m[index].numel();
    return GNNMP_OK;
}

extern "C" int gnnmp_smoother_create(gnnmp_smoother** out, const gnnmp_smoother_dims* dims, const float* weights_host,
                                     size_t n_floats, int device) {
    if (!out || !dims || !weights_host) return GNNMP_ERR_NULL;
    if (!sm_dims_ok(*dims)) return GNNMP_ERR_DIMS;
    Blob B;
    B.man = smoother_manifest(*dims);
    B.base = weights_host;
    int64_t tot = 0;
    for (auto& e : B.man) { B.off.push_back(tot); tot += e.numel(); }
    if ((int64_t)n_floats != tot) return GNNMP_ERR_WEIGHTS;
    const int C = dims->config_size, D = dims->embed_size;
    gnnmp_smoother* h = new gnnmp_smoother();
    h->dims = *dims;
    h->device = device;
    h->w_dev = nullptr;
    h->w_raw_dev = nullptr;
    h->man = B.man; h->man_off = B.off; h->n_raw = tot;
    const int PR = dims->mlp_dtype;
    h->L = SmLayout::make(PR, D, C);
    const SmLayout& L = h->L;
    std::vector<float> P(L.total, 0.f);
    auto ptiles = [&](const float* w, int out_f, int ld, float* dst) {
        if (PR) pack_a_tiles_bf16(w, out_f, ld, 0, D, dst); else gnnmp_pack_a_tiles(w, out_f, ld, 0, D, dst);
    };
    auto W = [&](const std::string& n) { return B.get(n); };
    // fold eval-mode BatchNorm (eps 1e-5) into node_code.0:  y = (W x + b - mean) * g + beta,  g = gamma / sqrt(var + eps)
    {
        const float *w0 = W("node_code.0.weight"), *b0 = W("node_code.0.bias"), *ga = W("node_code.1.weight"),
                    *be = W("node_code.1.bias"), *mu = W("node_code.1.running_mean"), *va = W("node_code.1.running_var");
        const int K = C + 3;
        std::vector<float> wf((size_t)D * K), bf(D);
        for (int i = 0; i < D; ++i) {
            const float g = ga[i] / std::sqrt(va[i] + 1e-5f);
            for (int k = 0; k < K; ++k) wf[(size_t)i * K + k] = w0[(size_t)i * K + k] * g;
            bf[i] = (b0[i] - mu[i]) * g + be[i];
        }
        if (PR) pack_a_small_bf16(wf.data(), D, K, 0, K, P.data() + L.as0); else gnnmp_pack_a_small(wf.data(), D, K, 0, K, P.data() + L.as0);
        gnnmp_pack_vec(bf.data(), D, P.data() + L.b0);
    }
    ptiles(W("node_code.3.weight"), D, D, P.data() + L.w3);
    gnnmp_pack_vec(W("node_code.3.bias"), D, P.data() + L.b3);
    {
        const float* w1 = W("process.lin_0.0.weight");      // [x_j - x_i | x_j | x_i]  model_smoother.py:37
        std::vector<float> ws((size_t)D * D), wd((size_t)D * D);
        for (int i = 0; i < D; ++i)
            for (int k = 0; k < D; ++k) {
                const float a = w1[(size_t)i * 3 * D + k], b = w1[(size_t)i * 3 * D + D + k], c = w1[(size_t)i * 3 * D + 2 * D + k];
                ws[(size_t)i * D + k] = a + b;
                wd[(size_t)i * D + k] = c - a;
            }
        ptiles(ws.data(), D, D, P.data() + L.wsrc);
        ptiles(wd.data(), D, D, P.data() + L.wdst);
        gnnmp_pack_vec(W("process.lin_0.0.bias"), D, P.data() + L.b00);
    }
    ptiles(W("process.lin_0.2.weight"), D, D, P.data() + L.w02);
    gnnmp_pack_vec(W("process.lin_0.2.bias"), D, P.data() + L.b02);
    ptiles(W("process.lin_1.0.weight"), D, D, P.data() + L.w10);
    gnnmp_pack_vec(W("process.lin_1.0.bias"), D, P.data() + L.b10);
    ptiles(W("process.lin_1.2.weight"), D, D, P.data() + L.w12);
    gnnmp_pack_vec(W("process.lin_1.2.bias"), D, P.data() + L.b12);
    {
        std::vector<float> ws((size_t)32 * D, 0.f), bs(32, 0.f);
        const float *w = W("smooth_node.weight"), *b = W("smooth_node.bias");
        for (int i = 0; i < C; ++i) {
            for (int k = 0; k < D; ++k) ws[(size_t)i * D + k] = w[(size_t)i * D + k];
            bs[i] = b[i];
        }
        ptiles(ws.data(), 32, D, P.data() + L.ws);
        gnnmp_pack_vec(bs.data(), 32, P.data() + L.bs);
    }
    int prev_dev = -1;
    (void)hipGetDevice(&prev_dev);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void**)&h->w_dev, P.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->w_dev, P.data(), P.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&h->w_raw_dev, (size_t)tot * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->w_raw_dev, weights_host, (size_t)tot * sizeof(float), hipMemcpyHostToDevice);
    if (prev_dev >= 0 && prev_dev != device) (void)hipSetDevice(prev_dev);
    if (e != hipSuccess) {
        if (h->w_dev) (void)hipFree(h->w_dev);
        if (h->w_raw_dev) (void)hipFree(h->w_raw_dev);
        delete h;
        return hip_fail(e);
    }
    *out = h;
    return GNNMP_OK;
}

extern "C" int gnnmp_smoother_destroy(gnnmp_smoother* h) {
    if (!h) return GNNMP_ERR_NULL;
    if (h->w_dev) (void)hipFree(h->w_dev);
    if (h->w_raw_dev) (void)hipFree(h->w_raw_dev);
    delete h;
    return GNNMP_OK;
}

namespace {
struct SmCarve {
    int ecap, pcap;
    size_t cur, knn, e_src, e_dst, e_count, stat, seg_beg, seg_cnt, ff_beg, etile, ptile, ff_end, msg, tgt, tflag, tcnt, elist, plist, total;
};

bool sm_carve(const gnnmp_smoother* h, const gnnmp_smooth_batch* b, SmCarve& c) {
    if (b->n_problems < 1 || b->total_path < 0 || b->total_edges < 0 || b->total_free < 0 || b->total_collided < 0)
        return false;
    const int D = h->dims.embed_size, C = h->dims.config_size;
    const long long ecap = (long long)b->total_edges + (long long)kSmK * b->total_path + 64LL * b->n_problems + 32;
    const long long pcap = (long long)b->total_path + 64LL * b->n_problems + 32;
    if (ecap > 0x3fffffff || pcap > 0x3fffffff) return false;
    c.ecap = (int)((ecap + 31) / 32 * 32);
    c.pcap = (int)((pcap + 31) / 32 * 32);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    c.cur = take(sizeof(float) * (size_t)b->total_path * C);
    c.knn = take(sizeof(int) * (size_t)b->total_path * kSmK);
    c.e_src = take(sizeof(int) * c.ecap);
    c.e_dst = take(sizeof(int) * c.ecap);
    c.e_count = take(sizeof(int) * b->n_problems);
    c.stat = take(sizeof(int) * b->n_problems);                 // device-side status per problem (gnnmp_smoother_status)
    c.seg_beg = take(sizeof(int) * c.pcap);
    c.seg_cnt = take(sizeof(int) * c.pcap);
    c.ff_beg = o;
    c.etile = take(sizeof(int) * (c.ecap / 32));
    c.ptile = take(sizeof(int) * (c.pcap / 32));
    c.ff_end = o;
    c.msg = take(sizeof(float) * (size_t)c.ecap * D);
    c.tgt = take(sizeof(float) * (size_t)c.pcap * D);
    c.tflag = take(sizeof(int) * (c.pcap / 32));
    // compact lists of the tiles in use (the tile space is padded per problem): two pairs of counters (iteration parity) + the lists,
    // appended by the graph stage, read by the streamed-weights message kernel
    c.tcnt = take(sizeof(int) * 4);
    c.elist = take(sizeof(int) * (c.ecap / 32));
    c.plist = take(sizeof(int) * (c.pcap / 32));
    c.total = o;
    return true;
}
}  // namespace

extern "C" int gnnmp_smoother_workspace_bytes(const gnnmp_smoother* h, const gnnmp_smooth_batch* shape, size_t* bytes) {
    if (!h || !shape || !bytes) return GNNMP_ERR_NULL;
    SmCarve c;
    if (!sm_carve(h, shape, c)) return GNNMP_ERR_ARG;
    *bytes = c.total;
    return GNNMP_OK;
}

namespace gnnmp { bool sm_wants_tile_lists(int D, int P, int n_etiles); }      // smoother_kernels.hip
extern "C" int gnnmp_smoother_forward_ex(const gnnmp_smoother* h, const gnnmp_smooth_batch* b, int loop, float* out_path,
                                         void* ws, size_t ws_bytes, void* hip_stream, int32_t* status_out);
extern "C" int gnnmp_smoother_forward(const gnnmp_smoother* h, const gnnmp_smooth_batch* b, int loop, float* out_path,
                                      void* ws, size_t ws_bytes, void* hip_stream) {
    return gnnmp_smoother_forward_ex(h, b, loop, out_path, ws, ws_bytes, hip_stream, nullptr);
}
extern "C" int gnnmp_smoother_forward_ex(const gnnmp_smoother* h, const gnnmp_smooth_batch* b, int loop, float* out_path,
                                         void* ws, size_t ws_bytes, void* hip_stream, int32_t* status_out) {
    if (!h || !b || !ws || !out_path) return GNNMP_ERR_NULL;
    if (!b->path) return GNNMP_ERR_NULL;
    // ONE problem may be given by its totals alone (the four prefix pointers NULL): the reference's call has no prefix
    // arrays (model_smoother.py:104) and building them costs the caller a host-to-device copy per call
    const bool implicit = !b->path_ptr && !b->free_ptr && !b->coll_ptr && !b->edge_ptr;
    if (implicit ? b->n_problems != 1 : (!b->path_ptr || !b->free_ptr || !b->coll_ptr || !b->edge_ptr)) return GNNMP_ERR_NULL;
    if ((b->total_free > 0 && !b->free_pts) || (b->total_collided > 0 && !b->collided) ||
        (b->total_edges > 0 && !b->edge_index))
        return GNNMP_ERR_NULL;
    if (loop < 0) return GNNMP_ERR_ARG;
    if (b->max_samples > 2048) return GNNMP_ERR_DIMS;          // kNN keeps <= 32 samples per lane
    SmCarve c;
    if (!sm_carve(h, b, c)) return GNNMP_ERR_ARG;
    if (ws_bytes < c.total || (reinterpret_cast<uintptr_t>(ws) & 255)) return GNNMP_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int C = h->dims.config_size, D = h->dims.embed_size;
    SmParams p;
    p.B = b->n_problems; p.C = C; p.total_path = b->total_path; p.total_edges = b->total_edges;
    p.scale = h->dims.scale;
    p.path = b->path; p.free_pts = b->free_pts; p.collided = b->collided;
    p.edge_index = reinterpret_cast<const long long*>(b->edge_index);
    p.path_ptr = b->path_ptr; p.free_ptr = b->free_ptr; p.coll_ptr = b->coll_ptr; p.edge_ptr = b->edge_ptr;
    p.w = h->w_dev; p.L = h->L;
    p.cur = at<float>(ws, c.cur); p.cur_next = p.cur;
    p.knn = at<int>(ws, c.knn);
    p.e_src = at<int>(ws, c.e_src); p.e_dst = at<int>(ws, c.e_dst); p.e_count = at<int>(ws, c.e_count);
    p.stat = status_out ? reinterpret_cast<int*>(status_out) : at<int>(ws, c.stat);      // one word per problem (gnnmp_smoother_forward_ex)
    p.seg_beg = at<int>(ws, c.seg_beg); p.seg_cnt = at<int>(ws, c.seg_cnt);
    p.etile_prob = at<int>(ws, c.etile); p.ptile_prob = at<int>(ws, c.ptile);
    p.msg = at<float>(ws, c.msg);
    p.tgt = at<float>(ws, c.tgt); p.tgt_flag = at<int>(ws, c.tflag);
    p.tile_cnt = at<int>(ws, c.tcnt); p.elist = at<int>(ws, c.elist); p.plist = at<int>(ws, c.plist); p.parity = 0;
    { static const int no_tgt = getenv("GNNMP_SM_NO_TARGET_ROLE") ? atoi(getenv("GNNMP_SM_NO_TARGET_ROLE")) : 0; if (no_tgt) p.tgt_flag = nullptr; }      // experiments
    p.cand_cap = b->max_edges + kSmK * b->max_path;
    if (p.cand_cap < 1) p.cand_cap = 1;
    p.samp_cap = b->max_samples > 0 ? b->max_samples : 0; p.path_cap = b->max_path > 0 ? b->max_path : 0;
    if ((size_t)2 * p.cand_cap * sizeof(int) > 60000) return GNNMP_ERR_DIMS;
    p.n_etiles = c.ecap / 32; p.n_ptiles = c.pcap / 32;
    p.one_free = b->total_free; p.one_coll = b->total_collided;
    if (loop == 0) {                                         // nothing moves: out = (path / scale) * scale
        HIP_TRY(hipMemsetAsync(p.stat, 0, sizeof(int) * b->n_problems, st));
        HIP_TRY(launch_sm_init(b->total_path * C, p.scale, b->path, p.cur, st));
        HIP_TRY(launch_sm_final(b->total_path * C, p.scale, p.cur, out_path, st));
        return GNNMP_OK;
    }
    // three launches per iteration (graph stage = kNN + edge list, messages, path update; four when a problem's buffers exceed
    // the LDS share of the one-launch graph stage): the scaled working copy is written by the
    // first kNN launch, the tile maps by the edge-list kernel, the result by the last path-update launch
    if (gnnmp::sm_wants_tile_lists(D, h->dims.mlp_dtype, p.n_etiles))
        HIP_TRY(hipMemsetAsync(p.tile_cnt, 0, sizeof(int) * 4, st));  // the tile-list counters (then re-armed by the graph stage itself)
    else
        p.tile_cnt = nullptr;                                          // no lists: the graph stage skips the bookkeeping
    int force_fallback = 0;
    {   // GNNMP_SM_FORCE_FALLBACK=1|2|3: the d = 128 message kernels take their flag-timeout fallback on all / even / odd edge tiles
        // or rounds without polling (the tests; read per call)
        const char* env = getenv("GNNMP_SM_FORCE_FALLBACK");
        if (env) force_fallback = atoi(env);
    }
    for (int it = 0; it < loop; ++it) {
        p.init_from_path = it == 0 ? 1 : 0;
        p.out = it == loop - 1 ? out_path : nullptr;
        p.parity = it & 1;
        HIP_TRY(launch_sm_iter(D, h->dims.mlp_dtype, p, st, force_fallback));
    }
    return GNNMP_OK;
}


extern "C" int gnnmp_smoother_status_region(const gnnmp_smoother* h, const gnnmp_smooth_batch* shape, size_t* offset, size_t* bytes) {
    if (!h || !shape || !offset || !bytes) return GNNMP_ERR_NULL;
    SmCarve c;
    if (!sm_carve(h, shape, c)) return GNNMP_ERR_ARG;
    *offset = c.stat;
    *bytes = sizeof(int) * (size_t)shape->n_problems;
    return GNNMP_OK;
}

extern "C" int gnnmp_smoother_status_decode(const int32_t* words_host, int n_problems, int32_t* first_problem) {
    if (!words_host || n_problems < 0) return GNNMP_ERR_NULL;
    for (int b = 0; b < n_problems; ++b)
        if (words_host[b] != 0) { if (first_problem) *first_problem = b; return GNNMP_ERR_CAPS; }
    if (first_problem) *first_problem = -1;
    return GNNMP_OK;
}

extern "C" int gnnmp_smoother_status(const gnnmp_smoother* h, const gnnmp_smooth_batch* shape, const void* ws, size_t ws_bytes,
                                     void* hip_stream, int32_t* first_problem) {
    if (!h || !shape || !ws) return GNNMP_ERR_NULL;
    SmCarve c;
    if (!sm_carve(h, shape, c)) return GNNMP_ERR_ARG;
    if (ws_bytes < c.total) return GNNMP_ERR_WORKSPACE;
    std::vector<int32_t> host((size_t)shape->n_problems);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipMemcpyAsync(host.data(), static_cast<const char*>(ws) + c.stat, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return gnnmp_smoother_status_decode(host.data(), shape->n_problems, first_problem);
}


// =============================================================================================
// device-side graph construction (create_data counterpart, eval_gnn.py:159-164)
// =============================================================================================
namespace {
struct GbCarve { size_t nb_all, nb_free, zero_beg, cnt, cur, large_cnt, zero_end, off, ucnt, uoff, gtotal, bucket, total; };
bool gb_carve(const gnnmp_graph_batch* b, GbCarve& c) {
    if (b->n_graphs < 1 || b->total_nodes < 0 || b->k1_max < 1 || b->config_size < 1) return false;
    if ((long long)4 * b->k1_max * b->total_nodes > 0x3fffffffLL) return false;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    const size_t n = (size_t)(b->total_nodes > 0 ? b->total_nodes : 1);
    c.nb_all = take(sizeof(int) * n * b->k1_max);
    c.nb_free = take(sizeof(int) * n * b->k1_max);
    c.zero_beg = o;
    c.cnt = take(sizeof(int) * n);
    c.cur = take(sizeof(int) * n);
    c.large_cnt = take(sizeof(int));
    c.zero_end = o;
    c.off = take(sizeof(int) * n);
    c.ucnt = take(sizeof(int) * n);
    c.uoff = take(sizeof(int) * n);
    c.gtotal = take(sizeof(int) * b->n_graphs);
    c.bucket = take(sizeof(int) * n * 4 * b->k1_max);
    c.total = o;
    return true;
}
}  // namespace

extern "C" int gnnmp_graph_workspace_bytes(const gnnmp_graph_batch* b, size_t* bytes) {
    if (!b || !bytes) return GNNMP_ERR_NULL;
    GbCarve c;
    if (!gb_carve(b, c)) return GNNMP_ERR_ARG;
    *bytes = c.total;
    return GNNMP_OK;
}

extern "C" int gnnmp_graph_build(const gnnmp_graph_batch* b, int64_t* edge_index_out, int64_t out_cap,
                                 int32_t* edge_ptr_out, void* ws, size_t ws_bytes, void* hip_stream) {
    if (!b || !edge_index_out || !edge_ptr_out || !ws) return GNNMP_ERR_NULL;
    if (!b->v || !b->node_ptr || !b->n_free || !b->k1) return GNNMP_ERR_NULL;
    GbCarve c;
    if (!gb_carve(b, c)) return GNNMP_ERR_ARG;
    if (out_cap < 1) return GNNMP_ERR_ARG;           // columns beyond out_cap are dropped; edge_ptr_out holds the true counts
    if (ws_bytes < c.total || (reinterpret_cast<uintptr_t>(ws) & 255)) return GNNMP_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipMemsetAsync(at<char>(ws, c.zero_beg), 0, c.zero_end - c.zero_beg, st));
    GbParams p;
    p.G = b->n_graphs; p.C = b->config_size; p.total_nodes = b->total_nodes; p.kmax = b->k1_max;
    p.v = b->v; p.node_ptr = b->node_ptr; p.n_free = b->n_free; p.k1 = b->k1;
    p.nb_all = at<int>(ws, c.nb_all); p.nb_free = at<int>(ws, c.nb_free);
    p.cnt = at<int>(ws, c.cnt); p.cur = at<int>(ws, c.cur); p.off = at<int>(ws, c.off);
    p.ucnt = at<int>(ws, c.ucnt); p.uoff = at<int>(ws, c.uoff); p.gtotal = at<int>(ws, c.gtotal);
    p.bucket = at<int>(ws, c.bucket);
    p.large_cnt = at<int>(ws, c.large_cnt); p.large = p.uoff;      // (uoff is first written after the kNN launches)
    p.edge_ptr = edge_ptr_out;
    p.edge_index = reinterpret_cast<long long*>(edge_index_out);
    p.out_cap = out_cap;
    if (b->total_nodes > 0) HIP_TRY(launch_graph_build(p, st));
    return GNNMP_OK;
}


// =============================================================================================
// device-side explore stage for 2-D mazes (eval_gnn.py:198-233 + environment/maze_env.py:270-326)
// =============================================================================================
namespace {
struct MzCarve { size_t in_ptr, cnt, in_rec, pos, prev, rb_val, rb_src, rb_eid, total; };
bool mz_carve(const gnnmp_maze_batch* b, MzCarve& c) {
    if (b->n_problems < 1 || b->total_nodes < 0 || b->total_edges < 0 || b->width < 1) return false;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    const size_t n = (size_t)b->total_nodes + b->n_problems + 1, e = (size_t)(b->total_edges > 0 ? b->total_edges : 1);
    c.in_ptr = take(sizeof(int) * n);
    c.cnt = take(sizeof(int) * n);
    c.in_rec = take(sizeof(int) * 2 * e);
    c.pos = take(sizeof(int) * n);
    c.prev = take(sizeof(int) * n);
    c.rb_val = take(sizeof(float) * n);
    c.rb_src = take(sizeof(int) * n);
    c.rb_eid = take(sizeof(int) * n);
    c.total = o;
    return true;
}
}  // namespace

extern "C" int gnnmp_maze_explore_workspace_bytes(const gnnmp_maze_batch* b, size_t* bytes) {
    if (!b || !bytes) return GNNMP_ERR_NULL;
    MzCarve c;
    if (!mz_carve(b, c)) return GNNMP_ERR_ARG;
    *bytes = c.total;
    return GNNMP_OK;
}

extern "C" int gnnmp_maze_explore_ex(const gnnmp_maze_batch* b, int32_t dim, const gnnmp_maze_resume* resume,
                                     int32_t* success, int32_t* n_explored, int32_t* explored, int32_t* n_pairs,
                                     int32_t* explored_edges, int32_t* path_len, int32_t* path, int64_t* checks,
                                     int32_t* prev_out, void* ws, size_t ws_bytes, void* hip_stream) {
    if (!b || !success || !n_explored || !explored || !n_pairs || !explored_edges || !path_len || !path || !checks || !ws)
        return GNNMP_ERR_NULL;
    if (!b->v || !b->node_ptr || !b->edge_ptr || !b->n_free || !b->maps || !b->goal_states) return GNNMP_ERR_NULL;
    if (b->total_edges > 0 && (!b->edge_index || !b->scores)) return GNNMP_ERR_NULL;
    if (dim != 2 && dim != 3) return GNNMP_ERR_DIMS;
    const bool res = resume && resume->n_explored;
    if (res && (!resume->explored || !resume->prev || !resume->n_pairs || !resume->pairs || !resume->pair_ptr))
        return GNNMP_ERR_NULL;
    MzCarve c;
    if (!mz_carve(b, c)) return GNNMP_ERR_ARG;
    if (ws_bytes < c.total || (reinterpret_cast<uintptr_t>(ws) & 255)) return GNNMP_ERR_WORKSPACE;
    MazeParams p;
    p.B = b->n_problems; p.total_edges = b->total_edges; p.w = b->width;
    p.v = b->v; p.node_ptr = b->node_ptr; p.edge_ptr = b->edge_ptr; p.n_free = b->n_free;
    p.edge_index = reinterpret_cast<const long long*>(b->edge_index); p.scores = b->scores;
    p.maps = b->maps; p.goal_states = b->goal_states;
    p.in_ptr = at<int>(ws, c.in_ptr); p.cnt = at<int>(ws, c.cnt); p.in_rec = at<int2>(ws, c.in_rec);
    p.pos = at<int>(ws, c.pos); p.prev = at<int>(ws, c.prev);
    p.rb_val = at<float>(ws, c.rb_val); p.rb_src = at<int>(ws, c.rb_src); p.rb_eid = at<int>(ws, c.rb_eid);
    p.success = success; p.n_explored = n_explored; p.explored = explored; p.n_pairs = n_pairs;
    p.explored_edges = explored_edges; p.path_len = path_len; p.path = path;
    p.checks = reinterpret_cast<long long*>(checks);
    p.dim = dim;
    p.n_explored0 = res ? resume->n_explored : nullptr; p.explored0 = res ? resume->explored : nullptr;
    p.prev0 = res ? resume->prev : nullptr; p.n_pairs0 = res ? resume->n_pairs : nullptr;
    p.pairs0 = res ? resume->pairs : nullptr; p.pair_ptr0 = res ? resume->pair_ptr : nullptr;
    p.prev_out = prev_out;
    HIP_TRY(launch_maze_explore(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_maze_explore(const gnnmp_maze_batch* b, int32_t* success, int32_t* n_explored, int32_t* explored,
                                  int32_t* n_pairs, int32_t* explored_edges, int32_t* path_len, int32_t* path,
                                  int64_t* checks, void* ws, size_t ws_bytes, void* hip_stream) {
    return gnnmp_maze_explore_ex(b, 2, nullptr, success, n_explored, explored, n_pairs, explored_edges, path_len, path, checks,
                                 nullptr, ws, ws_bytes, hip_stream);
}

extern "C" int gnnmp_maze_steer(int32_t n_problems, int32_t total_path, int32_t width, const double* maps,
                                const int32_t* path_ptr, const float* old_path, const float* new_path, float* out_path,
                                float* tmp, int64_t* checks, void* hip_stream) {
    if (!maps || !path_ptr || !checks) return GNNMP_ERR_NULL;
    if (n_problems < 1 || total_path < 0 || width < 1) return GNNMP_ERR_ARG;
    if (total_path > 0 && (!old_path || !new_path || !out_path || !tmp)) return GNNMP_ERR_NULL;
    if (out_path == old_path || out_path == new_path) return GNNMP_ERR_ARG;
    MazeSteerParams p;
    p.B = n_problems; p.w = width; p.maps = maps; p.path_ptr = path_ptr;
    p.old_path = old_path; p.new_path = new_path; p.out_path = out_path; p.tmp = tmp;
    p.checks = reinterpret_cast<long long*>(checks);
    HIP_TRY(launch_maze_steer(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_stick_steer(int32_t n_problems, int32_t total_path, int32_t width, const double* maps,
                                 const int32_t* path_ptr, const float* old_path, const float* new_path, float* out_path,
                                 float* tmp, int64_t* checks, int32_t* status, void* hip_stream) {
    if (!maps || !path_ptr || !checks || !status) return GNNMP_ERR_NULL;
    if (n_problems < 1 || total_path < 0 || width < 1) return GNNMP_ERR_ARG;
    if (total_path > 0 && (!old_path || !new_path || !out_path || !tmp)) return GNNMP_ERR_NULL;
    if (out_path == old_path || out_path == new_path) return GNNMP_ERR_ARG;
    MazeSteerParams p;
    p.B = n_problems; p.w = width; p.maps = maps; p.path_ptr = path_ptr;
    p.old_path = old_path; p.new_path = new_path; p.out_path = out_path; p.tmp = tmp;
    p.checks = reinterpret_cast<long long*>(checks);
    p.dim = 3; p.status = status;
    HIP_TRY(launch_maze_steer(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_maze_sample(const gnnmp_maze_sample_batch* b, int64_t* cursor, float* v_out, int32_t* node_ptr_out,
                                 int32_t* used_out, int32_t* ok_out, void* hip_stream) {
    if (!b || !cursor || !v_out || !node_ptr_out || !used_out || !ok_out) return GNNMP_ERR_NULL;
    if (!b->attempts || !b->maps || !b->init_states || !b->goal_states) return GNNMP_ERR_NULL;
    if (b->n_problems < 1 || b->width < 1 || b->n_free < 1 || b->n_attempts < 0) return GNNMP_ERR_ARG;
    MazeSampleParams p;
    p.B = b->n_problems; p.w = b->width; p.n = b->n_free;
    p.attempts = b->attempts; p.M = b->n_attempts;
    p.maps = b->maps; p.init_states = b->init_states; p.goal_states = b->goal_states;
    p.v = v_out; p.node_ptr = node_ptr_out; p.used = used_out;
    p.cursor = reinterpret_cast<long long*>(cursor); p.ok = ok_out;
    HIP_TRY(launch_maze_sample(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_stick_sample(const gnnmp_maze_sample_batch* b, int64_t* cursor, float* v_out, int32_t* node_ptr_out,
                                  int32_t* used_out, int64_t* checks_out, int32_t* ok_out, void* hip_stream) {
    if (!b || !cursor || !v_out || !node_ptr_out || !used_out || !checks_out || !ok_out) return GNNMP_ERR_NULL;
    if (!b->attempts || !b->maps || !b->init_states || !b->goal_states) return GNNMP_ERR_NULL;
    if (b->n_problems < 1 || b->width < 1 || b->n_free < 1 || b->n_attempts < 0) return GNNMP_ERR_ARG;
    MazeSampleParams p;
    p.B = b->n_problems; p.w = b->width; p.n = b->n_free;
    p.attempts = b->attempts; p.M = b->n_attempts;
    p.maps = b->maps; p.init_states = b->init_states; p.goal_states = b->goal_states;
    p.v = v_out; p.node_ptr = node_ptr_out; p.used = used_out;
    p.checks = reinterpret_cast<long long*>(checks_out);
    p.cursor = reinterpret_cast<long long*>(cursor); p.ok = ok_out;
    HIP_TRY(launch_stick_sample(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_maze_sample_streams(const gnnmp_maze_streams_batch* b, int32_t dim, float* free_pool, int32_t* n_free,
                                         float* coll_pool, int32_t* n_coll, int32_t* used_out, int64_t* checks_out,
                                         int32_t* status_out, void* hip_stream) {
    if (dim != 2 && dim != 3) return GNNMP_ERR_DIMS;
    if (!b || !free_pool || !n_free || !coll_pool || !n_coll || !used_out || !checks_out || !status_out) return GNNMP_ERR_NULL;
    if (!b->attempts || !b->att_ptr || !b->maps || !b->init_states || !b->goal_states) return GNNMP_ERR_NULL;
    if (b->n_problems < 1 || b->width < 1 || b->n_free < 1 || b->cap < b->n_free || b->n_attempts < 0) return GNNMP_ERR_ARG;
    if (b->att_ptr_host) {
        if (b->att_ptr_host[0] < 0 || b->att_ptr_host[b->n_problems] > b->n_attempts) return GNNMP_ERR_ARG;
        for (int i = 0; i < b->n_problems; ++i)
            if (b->att_ptr_host[i + 1] < b->att_ptr_host[i]) return GNNMP_ERR_ARG;
    }
    MazeStreamsParams p;
    p.B = b->n_problems; p.w = b->width; p.n = b->n_free; p.cap = b->cap; p.dim = dim;
    p.attempts = b->attempts; p.M = b->n_attempts; p.att_ptr = reinterpret_cast<const long long*>(b->att_ptr);
    p.maps = b->maps; p.init_states = b->init_states; p.goal_states = b->goal_states; p.active = b->active;
    p.free_pool = free_pool; p.coll_pool = coll_pool; p.n_free = n_free; p.n_coll = n_coll;
    p.used = used_out; p.checks = reinterpret_cast<long long*>(checks_out); p.status = status_out;
    HIP_TRY(launch_maze_sample_streams(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

namespace {
// finite by the exponent bits: the library is built with -fno-honor-nans, which lets the compiler fold std::isfinite(NaN)
bool finite_bits(double x) {
    uint64_t u;
    std::memcpy(&u, &x, sizeof u);
    return ((u >> 52) & 0x7ff) != 0x7ff;
}
}  // namespace

extern "C" int gnnmp_mt19937_seed(int32_t n_streams, const uint32_t* seeds, uint32_t* state, void* hip_stream) {
    if (!seeds || !state) return GNNMP_ERR_NULL;
    if (n_streams < 1) return GNNMP_ERR_ARG;
    HIP_TRY(launch_mt_seed(n_streams, seeds, state, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_mt19937_uniform(const gnnmp_mt_uniform_batch* b, uint32_t* state, double* out, int32_t commit,
                                     int32_t* status_out, void* hip_stream) {
    if (!b || !state || !status_out || !b->counts) return GNNMP_ERR_NULL;
    if (b->dim < 1 || b->dim > 3) return GNNMP_ERR_DIMS;
    if (out && !b->out_ptr) return GNNMP_ERR_NULL;
    if (b->n_streams < 1 || b->out_rows < 0 || (!out && !commit)) return GNNMP_ERR_ARG;
    double low[3] = {0.0, 0.0, 0.0}, range[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < b->dim; ++c) {
        if (!(finite_bits(b->low[c]) && finite_bits(b->range[c]))) return GNNMP_ERR_ARG;
        low[c] = b->low[c];
        range[c] = b->range[c];
    }
    MtUniformParams p;
    p.low0 = low[0]; p.low1 = low[1]; p.low2 = low[2]; p.range0 = range[0]; p.range1 = range[1]; p.range2 = range[2];
    p.n = b->n_streams; p.dim = b->dim; p.commit = commit ? 1 : 0; p.out_rows = b->out_rows;
    p.counts = b->counts; p.out_ptr = reinterpret_cast<const long long*>(b->out_ptr); p.active = b->active;
    p.state = state; p.out = out; p.status = status_out;
    HIP_TRY(launch_mt_uniform(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

namespace {
int rounds_state_check(const gnnmp_maze_rounds_state* s, bool trees) {
    if (!s) return GNNMP_ERR_NULL;
    if (!s->free_pool || !s->coll_pool || !s->n_free || !s->n_coll) return GNNMP_ERR_NULL;
    if (trees && (!s->tree_explored || !s->tree_prev || !s->tree_n_explored || !s->tree_pairs || !s->tree_n_pairs)) return GNNMP_ERR_NULL;
    if (s->n_problems < 1 || s->cap < 1 || s->pair_cap < 1 || (long long)s->n_problems * s->pair_cap > (1ll << 30)) return GNNMP_ERR_ARG;
    return GNNMP_OK;
}
}  // namespace

extern "C" int gnnmp_maze_rounds_gather(const gnnmp_maze_rounds_state* s, int32_t dim, const uint8_t* active, int32_t n_active,
                                        int64_t v_rows, float* v_out, int32_t* node_ptr_out, int32_t* n_free_out, int32_t* slot_out,
                                        const gnnmp_maze_resume* r, void* hip_stream) {
    if (dim != 2 && dim != 3) return GNNMP_ERR_DIMS;
    if (!v_out || !node_ptr_out || !n_free_out || !slot_out) return GNNMP_ERR_NULL;
    if (r && (!r->n_explored || !r->explored || !r->prev || !r->n_pairs || !r->pair_ptr)) return GNNMP_ERR_NULL;
    if (const int rc = rounds_state_check(s, r != nullptr)) return rc;
    if (v_rows < 0 || n_active < 1 || n_active > s->n_problems) return GNNMP_ERR_ARG;
    MazeGatherParams p;
    p.A = n_active; p.B = s->n_problems; p.dim = dim; p.cap = s->cap; p.pair_cap = s->pair_cap; p.v_rows = v_rows;
    p.free_pool = s->free_pool; p.coll_pool = s->coll_pool; p.n_free = s->n_free; p.n_coll = s->n_coll; p.active = active;
    p.v = v_out; p.node_ptr = node_ptr_out; p.n_free_out = n_free_out; p.slot_of = slot_out;
    p.tree_explored = s->tree_explored; p.tree_prev = s->tree_prev; p.tree_n_explored = s->tree_n_explored;
    p.tree_n_pairs = s->tree_n_pairs;
    // (the resume struct is const for its reader, gnnmp_maze_explore_ex; here its arrays are the outputs)
    p.res_n_explored = r ? const_cast<int*>(r->n_explored) : nullptr; p.res_explored = r ? const_cast<int*>(r->explored) : nullptr;
    p.res_prev = r ? const_cast<int*>(r->prev) : nullptr; p.res_n_pairs = r ? const_cast<int*>(r->n_pairs) : nullptr;
    p.res_pair_ptr = r ? const_cast<int*>(r->pair_ptr) : nullptr;
    HIP_TRY(launch_maze_rounds_gather(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_maze_rounds_carry(const gnnmp_maze_rounds_state* s, int32_t n_active, const int32_t* slot_of,
                                       const int32_t* node_ptr, const int32_t* edge_ptr, const int32_t* success,
                                       const int32_t* n_explored, const int32_t* explored, const int32_t* prev,
                                       const int32_t* n_pairs, const int32_t* explored_edges, const int32_t* path_len,
                                       const int32_t* path, const int64_t* checks, int32_t* status_out, void* hip_stream) {
    if (!node_ptr || !edge_ptr || !success || !n_explored || !explored || !prev || !n_pairs || !explored_edges || !path_len ||
        !path || !checks || !status_out)
        return GNNMP_ERR_NULL;
    if (const int rc = rounds_state_check(s, true)) return rc;
    if (!s->tree_success || !s->tree_path_len || !s->tree_path || !s->tree_checks) return GNNMP_ERR_NULL;
    if (n_active < 1 || n_active > s->n_problems) return GNNMP_ERR_ARG;
    MazeCarryParams p;
    p.A = n_active; p.B = s->n_problems; p.cap = s->cap; p.pair_cap = s->pair_cap;
    p.slot_of = slot_of; p.node_ptr = node_ptr; p.edge_ptr = edge_ptr;
    p.success = success; p.n_explored = n_explored; p.explored = explored; p.prev = prev; p.n_pairs = n_pairs;
    p.pairs = explored_edges; p.path_len = path_len; p.path = path; p.checks = reinterpret_cast<const long long*>(checks);
    p.tree_explored = s->tree_explored; p.tree_prev = s->tree_prev; p.tree_n_explored = s->tree_n_explored;
    p.tree_pairs = s->tree_pairs; p.tree_n_pairs = s->tree_n_pairs; p.tree_success = s->tree_success;
    p.tree_path_len = s->tree_path_len; p.tree_path = s->tree_path; p.tree_checks = reinterpret_cast<long long*>(s->tree_checks);
    p.status = status_out;
    HIP_TRY(launch_maze_rounds_carry(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

// =============================================================================================
// the LazySP baseline on maze problems (lazysp_kernels.hip; algorithm/lazy_sp.py:147-196)
// =============================================================================================
namespace {
int lazysp_state_check(const gnnmp_lazysp_state* s, bool lists) {
    if (!s) return GNNMP_ERR_NULL;
    if (!s->pool || !s->n_nodes) return GNNMP_ERR_NULL;
    if (lists && (!s->pairs || !s->pair_state || !s->n_pairs || !s->checks || !s->dijkstra_runs || !s->path_len || !s->path ||
                  !s->solved || !s->status))
        return GNNMP_ERR_NULL;
    if (s->n_problems < 1 || s->cap < 1 || s->pair_cap < 1 || (long long)s->n_problems * s->pair_cap > (1ll << 30)) return GNNMP_ERR_ARG;
    return GNNMP_OK;
}
size_t lsp_align(size_t x) { return (x + 255) & ~(size_t)255; }
struct LspCarve { size_t cost, flag, dist, prev, rb, total; };
LspCarve lsp_carve(int n_active, int cap, long long total_edges) {
    LspCarve c;
    const size_t nodes = (size_t)n_active * ((size_t)cap + 3);
    size_t off = 0;
    c.cost = off; off = lsp_align(off + sizeof(double) * (size_t)total_edges);
    c.flag = off; off = lsp_align(off + (size_t)total_edges);
    c.dist = off; off = lsp_align(off + sizeof(unsigned long long) * nodes);
    c.prev = off; off = lsp_align(off + sizeof(int) * nodes);
    c.rb = off;   off = lsp_align(off + sizeof(int) * nodes);
    c.total = off;
    return c;
}
}  // namespace

extern "C" int gnnmp_lazysp_pair_cap(int32_t batch, int32_t n_rounds, const int32_t* k1_by_round, int64_t* pair_cap) {
    if (!k1_by_round || !pair_cap) return GNNMP_ERR_NULL;
    if (batch < 1 || n_rounds < 1) return GNNMP_ERR_ARG;
    long long cap = 0;
    for (int r = 1; r <= n_rounds; ++r) {
        const long long n = 2 + (long long)r * batch, k1 = k1_by_round[r - 1];
        if (k1 < 1) return GNNMP_ERR_ARG;
        const long long by_k = (k1 < n ? k1 : n) * n, all = n * (n - 1) / 2;
        cap += by_k < all ? by_k : all;
        if (cap > (1ll << 30)) return GNNMP_ERR_ARG;
    }
    *pair_cap = cap < 1 ? 1 : cap;
    return GNNMP_OK;
}

extern "C" int gnnmp_lazysp_sample(const gnnmp_maze_streams_batch* b, int32_t dim, const gnnmp_lazysp_state* s, int32_t* used_out,
                                   int64_t* checks_out, int32_t* status_out, void* hip_stream) {
    if (dim != 2 && dim != 3) return GNNMP_ERR_DIMS;
    if (!b || !used_out || !checks_out || !status_out) return GNNMP_ERR_NULL;
    if (!b->attempts || !b->att_ptr || !b->maps || !b->init_states || !b->goal_states) return GNNMP_ERR_NULL;
    if (const int rc = lazysp_state_check(s, false)) return rc;
    if (!s->checks) return GNNMP_ERR_NULL;
    if (b->n_problems < 1 || b->n_problems != s->n_problems || b->width < 1 || b->n_free < 1 || s->cap < b->n_free || b->n_attempts < 0)
        return GNNMP_ERR_ARG;
    if (b->att_ptr_host) {
        if (b->att_ptr_host[0] < 0 || b->att_ptr_host[b->n_problems] > b->n_attempts) return GNNMP_ERR_ARG;
        for (int i = 0; i < b->n_problems; ++i)
            if (b->att_ptr_host[i + 1] < b->att_ptr_host[i]) return GNNMP_ERR_ARG;
    }
    LspSampleParams p;
    p.B = b->n_problems; p.w = b->width; p.n = b->n_free; p.cap = s->cap; p.dim = dim;
    p.attempts = b->attempts; p.M = b->n_attempts; p.att_ptr = reinterpret_cast<const long long*>(b->att_ptr);
    p.maps = b->maps; p.init_states = b->init_states; p.goal_states = b->goal_states; p.active = b->active;
    p.pool = s->pool; p.n_nodes = s->n_nodes; p.checks = reinterpret_cast<long long*>(s->checks);
    p.used = used_out; p.checks_out = reinterpret_cast<long long*>(checks_out); p.status = status_out;
    HIP_TRY(launch_lsp_sample(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_lazysp_gather(const gnnmp_lazysp_state* s, int32_t dim, int32_t n_active, const int32_t* slot_of,
                                   const int32_t* k1_table, int64_t v_rows, float* v_out, int32_t* node_ptr_out,
                                   int32_t* n_free_out, int32_t* k1_out, void* hip_stream) {
    if (dim != 2 && dim != 3) return GNNMP_ERR_DIMS;
    if (!slot_of || !k1_table || !v_out || !node_ptr_out || !n_free_out || !k1_out) return GNNMP_ERR_NULL;
    if (const int rc = lazysp_state_check(s, false)) return rc;
    if (v_rows < 0 || n_active < 1 || n_active > s->n_problems) return GNNMP_ERR_ARG;
    LspGatherParams p;
    p.A = n_active; p.B = s->n_problems; p.cap = s->cap; p.dim = dim; p.v_rows = v_rows;
    p.slot_of = slot_of; p.pool = s->pool; p.n_nodes = s->n_nodes; p.k1_table = k1_table;
    p.v = v_out; p.node_ptr = node_ptr_out; p.n_free_out = n_free_out; p.k1_out = k1_out;
    HIP_TRY(launch_lsp_gather(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_lazysp_workspace_bytes(int32_t n_active, int32_t cap, int64_t total_edges, size_t* bytes) {
    if (!bytes) return GNNMP_ERR_NULL;
    if (n_active < 1 || cap < 1 || total_edges < 0) return GNNMP_ERR_ARG;
    *bytes = lsp_carve(n_active, cap, total_edges).total;
    return GNNMP_OK;
}

extern "C" int gnnmp_lazysp_lds_nodes(void) { return lsp_lds_nodes(); }

extern "C" int gnnmp_lazysp_round(const gnnmp_lazysp_state* s, int32_t dim, int32_t n_active, const int32_t* slot_of,
                                  const int64_t* edge_index, int64_t total_edges, const int32_t* edge_ptr, const double* maps,
                                  int32_t width, void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (dim != 2 && dim != 3) return GNNMP_ERR_DIMS;
    if (!edge_index || !edge_ptr || !maps || !workspace) return GNNMP_ERR_NULL;
    if (const int rc = lazysp_state_check(s, true)) return rc;
    if (n_active < 1 || n_active > s->n_problems || width < 1 || total_edges < 0) return GNNMP_ERR_ARG;
    const LspCarve c = lsp_carve(n_active, s->cap, total_edges);
    if (workspace_bytes < c.total || (reinterpret_cast<uintptr_t>(workspace) & 255)) return GNNMP_ERR_WORKSPACE;
    char* ws = static_cast<char*>(workspace);
    LspRoundParams p;
    p.A = n_active; p.B = s->n_problems; p.cap = s->cap; p.pair_cap = s->pair_cap; p.dim = dim; p.w = width;
    p.total_edges = total_edges; p.slot_of = slot_of; p.edge_ptr = edge_ptr;
    p.edge_index = reinterpret_cast<const long long*>(edge_index); p.maps = maps;
    p.pool = s->pool; p.n_nodes = s->n_nodes; p.pairs = s->pairs; p.n_pairs = s->n_pairs; p.dijkstra_runs = s->dijkstra_runs;
    p.path_len = s->path_len; p.path = s->path; p.status = s->status; p.solved = s->solved; p.pair_state = s->pair_state;
    p.checks = reinterpret_cast<long long*>(s->checks);
    p.ws_cost = reinterpret_cast<double*>(ws + c.cost); p.ws_flag = reinterpret_cast<unsigned char*>(ws + c.flag);
    p.ws_dist = reinterpret_cast<unsigned long long*>(ws + c.dist); p.ws_prev = reinterpret_cast<int*>(ws + c.prev);
    p.ws_rb = reinterpret_cast<int*>(ws + c.rb);
    HIP_TRY(launch_lsp_round(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

// =============================================================================================
// the RRT* baseline on maze problems (rrtstar_kernels.hip; algorithm/tsa.py:12-139, 222-281)
// =============================================================================================
namespace {
struct RrtCarve { size_t x, y, z, c, f, total; };
RrtCarve rrt_carve(int n_problems, int t_max) {
    RrtCarve c{0, 0, 0, 0, 0, 0};
    if ((long long)t_max + 1 <= rrtstar_lds_nodes()) return c;   // the node state fits LDS: no workspace
    const size_t nodes = (size_t)n_problems * ((size_t)t_max + 1);
    size_t off = 0;
    c.x = off; off = lsp_align(off + sizeof(double) * nodes);
    c.y = off; off = lsp_align(off + sizeof(double) * nodes);
    c.z = off; off = lsp_align(off + sizeof(double) * nodes);
    c.c = off; off = lsp_align(off + sizeof(double) * nodes);
    c.f = off; off = lsp_align(off + nodes);
    c.total = off;
    return c;
}
}  // namespace

extern "C" int gnnmp_rrtstar_workspace_bytes(int32_t n_problems, int32_t t_max, size_t* bytes) {
    if (!bytes) return GNNMP_ERR_NULL;
    if (n_problems < 1 || t_max < 1 || t_max == INT32_MAX) return GNNMP_ERR_ARG;
    *bytes = rrt_carve(n_problems, t_max).total;
    return GNNMP_OK;
}

extern "C" int gnnmp_rrtstar_lds_nodes(void) { return rrtstar_lds_nodes(); }

extern "C" int gnnmp_rrtstar_plan(const gnnmp_rrtstar_batch* b, const gnnmp_rrtstar_tree* t, void* workspace, size_t workspace_bytes,
                                  void* hip_stream) {
    if (!b || !t) return GNNMP_ERR_NULL;
    if (b->dim != 2 && b->dim != 3) return GNNMP_ERR_DIMS;
    if (!b->maps || !b->init_states || !b->goal_states || !b->draws) return GNNMP_ERR_NULL;
    if (!t->states || !t->parents || !t->rewired_parents || !t->flags || !t->costs || !t->path_lengths || !t->cumulated_checks ||
        !t->path || !t->n_nodes || !t->success || !t->last_iter || !t->used || !t->path_len || !t->status)
        return GNNMP_ERR_NULL;
    if (b->n_problems < 1 || b->width < 1 || b->t_max < 1 || b->t_max == INT32_MAX) return GNNMP_ERR_ARG;
    if (b->draws_per_problem < 2 + b->dim || b->draws_per_problem > INT32_MAX) return GNNMP_ERR_ARG;      // one iteration at least
    const RrtCarve c = rrt_carve(b->n_problems, b->t_max);
    if (c.total) {
        if (!workspace) return GNNMP_ERR_NULL;
        if (workspace_bytes < c.total || (reinterpret_cast<uintptr_t>(workspace) & 255)) return GNNMP_ERR_WORKSPACE;
    }
    char* ws = static_cast<char*>(workspace);
    RrtParams p;
    p.B = b->n_problems; p.w = b->width; p.t_max = b->t_max; p.stop = b->stop_when_success ? 1 : 0; p.dim = b->dim;
    p.draw_len = b->draws_per_problem;
    p.maps = b->maps; p.init_states = b->init_states; p.goal_states = b->goal_states; p.draws = b->draws;
    p.states = t->states; p.parents = t->parents; p.rewired = t->rewired_parents; p.flags = t->flags; p.costs = t->costs;
    p.path_lengths = t->path_lengths; p.cum_checks = reinterpret_cast<long long*>(t->cumulated_checks); p.path = t->path;
    p.n_nodes = t->n_nodes; p.success = t->success; p.last_iter = t->last_iter; p.used = t->used; p.path_len = t->path_len;
    p.status = t->status;
    p.ws_x = reinterpret_cast<double*>(ws + c.x); p.ws_y = reinterpret_cast<double*>(ws + c.y);
    p.ws_z = reinterpret_cast<double*>(ws + c.z); p.ws_c = reinterpret_cast<double*>(ws + c.c);
    p.ws_f = reinterpret_cast<unsigned char*>(ws + c.f);
    HIP_TRY(launch_rrtstar_plan(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

// =============================================================================================
// the BIT* baseline on maze problems (bitstar_kernels.hip; algorithm/bit_star.py:18-334)
// =============================================================================================
namespace {
struct BitCarve { size_t eval, esrc, etgt, vval, flag, total; };
BitCarve bit_carve(int n_problems, int n_nodes, long long edge_cap) {
    BitCarve c{0, 0, 0, 0, 0, 0};
    const size_t edges = (size_t)n_problems * (size_t)edge_cap, nodes = (size_t)n_problems * (size_t)n_nodes;
    size_t off = 0;
    c.eval = off; off = lsp_align(off + sizeof(double) * edges);
    c.esrc = off; off = lsp_align(off + sizeof(int) * edges);
    c.etgt = off; off = lsp_align(off + sizeof(int) * edges);
    c.vval = off; off = lsp_align(off + sizeof(double) * nodes);
    c.flag = off; off = lsp_align(off + nodes);
    c.total = off;
    return c;
}
bool bit_sizes_ok(int n_problems, int n_nodes, long long edge_cap) {
    return n_problems >= 1 && n_nodes >= 3 && edge_cap >= 1 && edge_cap <= (long long)n_nodes * (n_nodes - 1);
}
}  // namespace

extern "C" int gnnmp_bitstar_sample(const gnnmp_maze_streams_batch* b, int32_t dim, int32_t n_batches, double* pool,
                                    int64_t* used_by_batch, int64_t* checks_by_batch, int32_t* status_out, void* hip_stream) {
    if (dim != 2 && dim != 3) return GNNMP_ERR_DIMS;
    if (!b || !pool || !used_by_batch || !checks_by_batch || !status_out) return GNNMP_ERR_NULL;
    if (!b->attempts || !b->att_ptr || !b->maps || !b->init_states || !b->goal_states) return GNNMP_ERR_NULL;
    if (b->n_problems < 1 || b->width < 1 || b->n_free < 1 || n_batches < 1 || b->n_attempts < 0) return GNNMP_ERR_ARG;
    if ((long long)b->cap < 2 + (long long)n_batches * b->n_free) return GNNMP_ERR_ARG;
    if (b->att_ptr_host) {
        if (b->att_ptr_host[0] < 0 || b->att_ptr_host[b->n_problems] > b->n_attempts) return GNNMP_ERR_ARG;
        for (int i = 0; i < b->n_problems; ++i)
            if (b->att_ptr_host[i + 1] < b->att_ptr_host[i]) return GNNMP_ERR_ARG;
    }
    BitSampleParams p;
    p.B = b->n_problems; p.w = b->width; p.batch = b->n_free; p.n_batches = n_batches; p.rows = b->cap; p.dim = dim;
    p.attempts = b->attempts; p.M = b->n_attempts; p.att_ptr = reinterpret_cast<const long long*>(b->att_ptr);
    p.maps = b->maps; p.init_states = b->init_states; p.goal_states = b->goal_states; p.active = b->active;
    p.pool = pool; p.used_by_batch = reinterpret_cast<long long*>(used_by_batch);
    p.checks_by_batch = reinterpret_cast<long long*>(checks_by_batch); p.status = status_out;
    HIP_TRY(launch_bit_sample(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_bitstar_workspace_bytes(int32_t n_problems, int32_t n_nodes, int64_t edge_cap, size_t* bytes) {
    if (!bytes) return GNNMP_ERR_NULL;
    if (!bit_sizes_ok(n_problems, n_nodes, edge_cap)) return GNNMP_ERR_ARG;
    *bytes = bit_carve(n_problems, n_nodes, edge_cap).total;
    return GNNMP_OK;
}

extern "C" int gnnmp_bitstar_lds_nodes(void) { return bit_lds_nodes(); }

extern "C" int gnnmp_bitstar_plan(const gnnmp_bitstar_batch* b, const gnnmp_bitstar_result* r, void* workspace, size_t workspace_bytes,
                                  void* hip_stream) {
    if (!b || !r) return GNNMP_ERR_NULL;
    if (b->dim != 2 && b->dim != 3) return GNNMP_ERR_DIMS;
    if (!b->maps || !b->pool || !b->r_by_batch || !b->checks_by_batch) return GNNMP_ERR_NULL;
    if (!r->g || !r->parents || !r->vertices || !r->path || !r->n_vertices || !r->batches_run || !r->success || !r->path_len ||
        !r->status || !r->counters)
        return GNNMP_ERR_NULL;
    if (b->width < 1 || b->batch < 1 || b->n_batches < 1 || (b->flags & ~1)) return GNNMP_ERR_ARG;
    if ((long long)b->n_nodes < 2 + (long long)b->n_batches * b->batch) return GNNMP_ERR_ARG;
    if (!bit_sizes_ok(b->n_problems, b->n_nodes, b->edge_cap)) return GNNMP_ERR_ARG;
    if (!workspace) return GNNMP_ERR_NULL;
    const BitCarve c = bit_carve(b->n_problems, b->n_nodes, b->edge_cap);
    if (workspace_bytes < c.total || (reinterpret_cast<uintptr_t>(workspace) & 255)) return GNNMP_ERR_WORKSPACE;
    char* ws = static_cast<char*>(workspace);
    BitPlanParams p;
    p.B = b->n_problems; p.w = b->width; p.batch = b->batch; p.n_batches = b->n_batches; p.rows = b->n_nodes; p.dim = b->dim;
    p.flags = b->flags; p.edge_cap = b->edge_cap;
    p.maps = b->maps; p.pool = b->pool; p.r_by_batch = b->r_by_batch;
    p.checks_by_batch = reinterpret_cast<const long long*>(b->checks_by_batch);
    p.g = r->g; p.parents = r->parents; p.vertices = r->vertices; p.path = r->path; p.n_vertices = r->n_vertices;
    p.batches_run = r->batches_run; p.success = r->success; p.path_len = r->path_len; p.status = r->status;
    p.counters = reinterpret_cast<long long*>(r->counters);
    p.ws_eval = reinterpret_cast<double*>(ws + c.eval); p.ws_esrc = reinterpret_cast<int*>(ws + c.esrc);
    p.ws_etgt = reinterpret_cast<int*>(ws + c.etgt); p.ws_vval = reinterpret_cast<double*>(ws + c.vval);
    p.ws_flag = reinterpret_cast<unsigned char*>(ws + c.flag);
    HIP_TRY(launch_bit_plan(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

// =============================================================================================
// the NEXT planning network on maze problems (next_kernels.hip; next_model/model2D.py:84-210)
// =============================================================================================
extern "C" int gnnmp_next_weights_floats(int32_t dim, size_t* n_floats) {
    if (!n_floats) return GNNMP_ERR_NULL;
    if (dim != 2 && dim != 3) return GNNMP_ERR_DIMS;
    *n_floats = next_weights_floats();
    return GNNMP_OK;
}

extern "C" int gnnmp_next_pb_forward(const gnnmp_next_pb* d, void* hip_stream) {
    if (!d) return GNNMP_ERR_NULL;
    if (d->dim != 2 && d->dim != 3) return GNNMP_ERR_DIMS;
    if (d->width != 15) return GNNMP_ERR_DIMS;
    if (d->n_problems < 0 || d->iters < 0) return GNNMP_ERR_ARG;
    if (!d->maps || !d->goals || !d->weights || !d->pb_rep) return GNNMP_ERR_NULL;
    if (d->n_problems == 0) return GNNMP_OK;
    NextPbParams p;
    p.B = d->n_problems; p.dim = d->dim; p.iters = d->iters;
    p.maps = d->maps; p.goals = d->goals; p.weights = d->weights; p.pb_rep = d->pb_rep;
    HIP_TRY(launch_next_pb_forward(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_next_state_forward(const gnnmp_next_states* d, void* hip_stream) {
    if (!d) return GNNMP_ERR_NULL;
    if (d->dim != 2 && d->dim != 3) return GNNMP_ERR_DIMS;
    if (d->width != 15) return GNNMP_ERR_DIMS;
    if (d->n_states < 0 || d->n_problems < 0) return GNNMP_ERR_ARG;
    if (!d->states || !d->problem_of_state || !d->pb_rep || !d->weights || !d->y || !d->status) return GNNMP_ERR_NULL;
    if (d->n_states == 0) return GNNMP_OK;
    NextStateParams p;
    p.S = d->n_states; p.B = d->n_problems; p.dim = d->dim;
    p.states = d->states; p.problem_of_state = d->problem_of_state; p.pb_rep = d->pb_rep; p.weights = d->weights; p.y = d->y;
    p.status = d->status;
    HIP_TRY(launch_next_state_forward(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

// =============================================================================================
// training the NEXT network on maze problems (next_train_kernels.hip).  One order of checks for every entry point: the struct,
// dims, negative counts, NULL arrays, then the no-work return BEFORE ANY HIP CALL (it writes nothing), then the workspace.
// =============================================================================================
extern "C" int gnnmp_next_train_workspace_bytes(int32_t n_problems, int32_t iters, int32_t n_states, size_t* bytes) {
    if (!bytes) return GNNMP_ERR_NULL;
    if (n_problems < 0 || iters < 0 || n_states < 0) return GNNMP_ERR_ARG;
    NextTrainCarve c;
    next_train_carve(n_problems, iters, n_states, c);
    *bytes = c.total;
    return GNNMP_OK;
}

extern "C" int gnnmp_next_weights_t_floats(int32_t dim, size_t* n_floats) {
    if (!n_floats) return GNNMP_ERR_NULL;
    if (dim != 2 && dim != 3) return GNNMP_ERR_DIMS;
    *n_floats = next_weights_t_floats();
    return GNNMP_OK;
}

static int next_train_ws(int32_t B, int32_t iters, int32_t S, const void* ws, size_t ws_bytes, NextTrainCarve& c) {
    next_train_carve(B, iters, S, c);
    if (ws_bytes < c.total || (reinterpret_cast<uintptr_t>(ws) & 255)) return GNNMP_ERR_WORKSPACE;
    return GNNMP_OK;
}

extern "C" int gnnmp_next_train_forward(const gnnmp_next_train* d, void* hip_stream) {
    if (!d) return GNNMP_ERR_NULL;
    if (d->dim != 2 && d->dim != 3) return GNNMP_ERR_DIMS;
    if (d->width != 15) return GNNMP_ERR_DIMS;
    if (d->n_problems < 0 || d->n_states < 0 || d->iters < 0) return GNNMP_ERR_ARG;
    if (!d->maps || !d->goals || !d->states || !d->problem_of_state || !d->weights || !d->pb_rep || !d->y || !d->status || !d->workspace)
        return GNNMP_ERR_NULL;
    if (d->n_problems == 0) return GNNMP_OK;                   // no work: no HIP call, nothing written
    NextTrainCarve c;
    if (int rc = next_train_ws(d->n_problems, d->iters, d->n_states, d->workspace, d->workspace_bytes, c)) return rc;
    NextPbParams p;
    p.B = d->n_problems; p.dim = d->dim; p.iters = d->iters;
    p.maps = d->maps; p.goals = d->goals; p.weights = d->weights; p.pb_rep = d->pb_rep;
    NextStateParams q;
    q.S = d->n_states; q.B = d->n_problems; q.dim = d->dim;
    q.states = d->states; q.problem_of_state = d->problem_of_state; q.pb_rep = d->pb_rep; q.weights = d->weights; q.y = d->y;
    q.status = d->status;
    HIP_TRY(launch_next_train_forward(p, q, static_cast<char*>(d->workspace), c, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

static int next_train_bwd(const gnnmp_next_train_bwd* d, void* hip_stream, bool state_call) {
    if (!d) return GNNMP_ERR_NULL;
    if (d->dim != 2 && d->dim != 3) return GNNMP_ERR_DIMS;
    if (d->width != 15) return GNNMP_ERR_DIMS;
    if (d->n_problems < 0 || d->n_states < 0 || d->iters < 0) return GNNMP_ERR_ARG;
    if (!d->goals || !d->states || !d->problem_of_state || !d->weights || !d->weights_t || !d->pb_rep || !d->dy || !d->dpb_rep ||
        !d->dweights || !d->workspace)
        return GNNMP_ERR_NULL;
    if (d->n_problems == 0 || (state_call && d->n_states == 0)) return GNNMP_OK;       // no work: no HIP call, nothing written
    NextTrainBwdParams p;
    if (int rc = next_train_ws(d->n_problems, d->iters, d->n_states, d->workspace, d->workspace_bytes, p.c)) return rc;
    p.B = d->n_problems; p.S = d->n_states; p.dim = d->dim; p.iters = d->iters;
    p.goals = d->goals; p.states = d->states; p.problem_of_state = d->problem_of_state; p.weights = d->weights;
    p.weights_t = d->weights_t; p.pb_rep = d->pb_rep; p.dy = d->dy; p.dpb_rep = d->dpb_rep; p.dweights = d->dweights;
    p.ws = static_cast<char*>(d->workspace);
    if (state_call) HIP_TRY(launch_next_state_backward(p, static_cast<hipStream_t>(hip_stream)));
    else HIP_TRY(launch_next_pb_backward(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_next_state_backward(const gnnmp_next_train_bwd* d, void* hip_stream) { return next_train_bwd(d, hip_stream, true); }
extern "C" int gnnmp_next_pb_backward(const gnnmp_next_train_bwd* d, void* hip_stream) { return next_train_bwd(d, hip_stream, false); }

// =============================================================================================
// the replay of NEXT's training loop (next_replay_kernels.hip).  The order of checks of the training entry points: the structs,
// dims, negative counts, NULL arrays, then the no-work return BEFORE ANY HIP CALL (it writes nothing).  There is no workspace.
// =============================================================================================
static int next_replay_store(const gnnmp_next_replay* s, NextReplayStore& st) {
    st.dim = s->dim; st.cap_paths = s->cap_paths; st.cap_states = s->cap_states;
    st.states64 = s->states64; st.states32 = s->states32; st.actions = s->actions; st.values = s->values;
    st.path_ptr = s->path_ptr; st.problem = s->problem; st.counts = s->counts; st.status = s->status; st.pending = s->pending;
    return !s->states64 || !s->states32 || !s->actions || !s->values || !s->path_ptr || !s->problem || !s->counts || !s->status ||
                   !s->pending
               ? GNNMP_ERR_NULL
               : GNNMP_OK;
}

extern "C" int gnnmp_next_replay_append_trees(const gnnmp_next_replay* s, const gnnmp_next_replay_trees* t, void* hip_stream) {
    if (!s || !t) return GNNMP_ERR_NULL;
    if (s->dim != 2 && s->dim != 3) return GNNMP_ERR_DIMS;
    if (s->cap_paths < 0 || s->cap_states < 0 || t->n_problems < 0 || t->t_max < 0 || t->t_max == INT32_MAX) return GNNMP_ERR_ARG;
    NextReplayStore st;
    if (int rc = next_replay_store(s, st)) return rc;
    if (!t->states || !t->path || !t->path_len || !t->success || !t->problem_ids) return GNNMP_ERR_NULL;
    if (t->n_problems == 0) return GNNMP_OK;                   // no work: no HIP call, nothing written
    NextReplaySrc src;
    src.n = t->n_problems; src.t1 = t->t_max + 1; src.n_rows = 0; src.rows = t->states; src.path = t->path;
    src.path_len = t->path_len; src.success = t->success; src.ptr = nullptr; src.problem_ids = t->problem_ids;
    HIP_TRY(launch_next_replay_append(st, src, true, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_next_replay_append_paths(const gnnmp_next_replay* s, const gnnmp_next_replay_paths* q, void* hip_stream) {
    if (!s || !q) return GNNMP_ERR_NULL;
    if (s->dim != 2 && s->dim != 3) return GNNMP_ERR_DIMS;
    if (s->cap_paths < 0 || s->cap_states < 0 || q->n_paths < 0 || q->n_states < 0) return GNNMP_ERR_ARG;
    NextReplayStore st;
    if (int rc = next_replay_store(s, st)) return rc;
    if (!q->paths64 || !q->path_ptr || !q->problem_ids) return GNNMP_ERR_NULL;
    if (q->n_paths == 0) return GNNMP_OK;                      // no work: no HIP call, nothing written
    NextReplaySrc src;
    src.n = q->n_paths; src.t1 = 0; src.n_rows = q->n_states; src.rows = q->paths64; src.path = nullptr; src.path_len = nullptr;
    src.success = nullptr; src.ptr = q->path_ptr; src.problem_ids = q->problem_ids;
    HIP_TRY(launch_next_replay_append(st, src, false, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_next_path_loss(const gnnmp_next_path_loss_desc* d, void* hip_stream) {
    if (!d) return GNNMP_ERR_NULL;
    if (d->dim != 2 && d->dim != 3) return GNNMP_ERR_DIMS;
    if (d->n_paths < 0 || d->n_states < 0 || d->divisor < 1) return GNNMP_ERR_ARG;
    if (!d->y || !d->actions || !d->values || !d->ptr || (d->loss && !d->terms)) return GNNMP_ERR_NULL;
    if (d->n_paths == 0 || (!d->terms && !d->dy)) return GNNMP_OK;          // no work: no HIP call, nothing written
    NextPathLossParams p;
    p.G = d->n_paths; p.S = d->n_states; p.dim = d->dim; p.divisor = d->divisor;
    p.y = d->y; p.actions = d->actions; p.values = d->values; p.ptr = d->ptr; p.terms = d->terms; p.loss = d->loss; p.dy = d->dy;
    HIP_TRY(launch_next_path_loss(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

// =============================================================================================
// the replay of the smoother's training loop (smoother_replay_kernels.hip).  The same order of checks: the structs, config_size,
// negative counts, NULL arrays (the store's first), then the no-work return BEFORE ANY HIP CALL (it writes nothing).
// =============================================================================================
static bool smooth_replay_dims_ok(int32_t C) { return C >= 2 && C <= 14; }

static bool smooth_replay_counts_bad(const gnnmp_smooth_replay* s) {
    return s->cap_samples < 0 || s->cap_path_rows < 0 || s->cap_free_rows < 0 || s->cap_coll_rows < 0 || s->epoch < 0 ||
           s->cap_samples == INT32_MAX;
}

static int smooth_replay_store(const gnnmp_smooth_replay* s, SmoothReplayStore& st) {
    st.C = s->config_size; st.cap_samples = s->cap_samples; st.cap_path = s->cap_path_rows; st.cap_free = s->cap_free_rows;
    st.cap_coll = s->cap_coll_rows; st.epoch = s->epoch;
    st.path = s->path; st.target = s->target; st.free_pts = s->free_pts; st.coll = s->collided;
    st.path_ptr = s->path_ptr; st.free_ptr = s->free_ptr; st.coll_ptr = s->coll_ptr; st.problem = s->problem;
    st.counts = s->counts; st.status = s->status; st.pending = s->pending;
    return !s->path || !s->target || !s->free_pts || !s->collided || !s->path_ptr || !s->free_ptr || !s->coll_ptr || !s->problem ||
                   !s->counts || !s->status || !s->pending
               ? GNNMP_ERR_NULL
               : GNNMP_OK;
}

extern "C" int gnnmp_smooth_replay_append(const gnnmp_smooth_replay* s, const gnnmp_smooth_replay_src* q, void* hip_stream) {
    if (!s || !q) return GNNMP_ERR_NULL;
    if (!smooth_replay_dims_ok(s->config_size)) return GNNMP_ERR_DIMS;
    if (smooth_replay_counts_bad(s) || q->n_samples < 0 || q->total_path < 0 || q->total_nodes < 0 || q->take_upper < 0 ||
        q->take_upper > q->n_samples)
        return GNNMP_ERR_ARG;
    SmoothReplayStore st;
    if (int rc = smooth_replay_store(s, st)) return rc;
    if (!q->path || !q->target || !q->v || !q->path_ptr || !q->node_ptr || !q->n_free || !q->take || !q->problem_ids)
        return GNNMP_ERR_NULL;
    if (q->n_samples == 0 || q->take_upper == 0) return GNNMP_OK;          // no work: no HIP call, nothing written
    SmoothReplaySrc src;
    src.B = q->n_samples; src.total_path = q->total_path; src.total_nodes = q->total_nodes; src.take_upper = q->take_upper;
    src.path = q->path; src.target = q->target; src.v = q->v; src.path_ptr = q->path_ptr; src.node_ptr = q->node_ptr;
    src.n_free = q->n_free; src.take = q->take; src.problem_ids = q->problem_ids;
    HIP_TRY(launch_smooth_replay_append(st, src, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_smooth_replay_gather(const gnnmp_smooth_replay* s, int32_t n_group, int32_t n_samples, const int32_t* idx,
                                          const gnnmp_smooth_batch* out, float* out_target, void* hip_stream) {
    if (!s || !out) return GNNMP_ERR_NULL;
    if (!smooth_replay_dims_ok(s->config_size)) return GNNMP_ERR_DIMS;
    if (smooth_replay_counts_bad(s) || n_group < 0 || n_samples < 0 || out->n_problems != n_group || out->total_path < 0 ||
        out->total_free < 0 || out->total_collided < 0 || out->total_edges < 0)
        return GNNMP_ERR_ARG;
    SmoothReplayStore st;
    if (int rc = smooth_replay_store(s, st)) return rc;
    if (!idx || !out->path || !out->free_pts || !out->collided || !out->edge_index || !out->path_ptr || !out->free_ptr ||
        !out->coll_ptr || !out->edge_ptr || !out_target)
        return GNNMP_ERR_NULL;
    if (n_group == 0) return GNNMP_OK;                                     // no work: no HIP call, nothing written
    SmoothGatherParams p;
    p.G = n_group; p.n_samples = n_samples; p.total_path = out->total_path; p.total_free = out->total_free;
    p.total_coll = out->total_collided; p.total_edges = out->total_edges; p.idx = idx;
    p.path = const_cast<float*>(out->path); p.target = out_target; p.free_pts = const_cast<float*>(out->free_pts);
    p.coll = const_cast<float*>(out->collided);
    p.edge_index = reinterpret_cast<long long*>(const_cast<int64_t*>(out->edge_index));
    p.path_ptr = const_cast<int32_t*>(out->path_ptr); p.free_ptr = const_cast<int32_t*>(out->free_ptr);
    p.coll_ptr = const_cast<int32_t*>(out->coll_ptr); p.edge_ptr = const_cast<int32_t*>(out->edge_ptr);
    HIP_TRY(launch_smooth_replay_gather(st, p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_smooth_path_loss(const gnnmp_smooth_path_loss_desc* d, void* hip_stream) {
    if (!d) return GNNMP_ERR_NULL;
    if (!smooth_replay_dims_ok(d->config_size)) return GNNMP_ERR_DIMS;
    if (d->n_paths < 0 || d->total_rows < 0 || d->divisor < 1) return GNNMP_ERR_ARG;
    if (!d->path_ptr || !d->pred || !d->target || !d->terms || !d->loss || !d->d_pred) return GNNMP_ERR_NULL;
    if (d->n_paths == 0) return GNNMP_OK;                                  // no work: no HIP call, nothing written
    SmoothPathLossParams p;
    p.G = d->n_paths; p.total_rows = d->total_rows; p.C = d->config_size; p.divisor = d->divisor;
    p.path_ptr = d->path_ptr; p.pred = d->pred; p.target = d->target; p.terms = d->terms; p.loss = d->loss; p.d_pred = d->d_pred;
    HIP_TRY(launch_smooth_path_loss(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

// =============================================================================================
// the explorer's training loop around one step (explorer_replay_kernels.hip).  The same order of checks: the structs, the dims,
// negative counts, NULL arrays (the store's first), then the no-work return BEFORE ANY HIP CALL (it writes nothing).
// =============================================================================================
extern "C" int gnnmp_episode_dataset_gather(const gnnmp_episode_dataset* s, int32_t n_group, const int32_t* idx,
                                            const gnnmp_episode_dataset_batch* out, void* hip_stream) {
    if (!s || !out) return GNNMP_ERR_NULL;
    if (s->config_size < 2 || s->config_size > 14 || s->obs_size < 1 || s->obs_size > 16) return GNNMP_ERR_DIMS;
    if (s->n_problems < 0 || s->total_nodes < 0 || s->total_edges < 0 || s->total_obs < 0 || n_group < 0 ||
        out->n_problems != n_group || out->total_nodes < 0 || out->total_edges < 0 || out->total_obs < 0)
        return GNNMP_ERR_ARG;
    if (!s->v || !s->points64 || !s->edge_index || !s->edge_free || !s->edge_cost || !s->obstacles || !s->node_ptr ||
        !s->edge_ptr || !s->obs_ptr || !s->status)
        return GNNMP_ERR_NULL;
    if (!idx || !out->v || !out->points64 || !out->edge_index || !out->edge_free || !out->edge_cost || !out->obstacles ||
        !out->node_ptr || !out->edge_ptr || !out->obs_ptr)
        return GNNMP_ERR_NULL;
    if (n_group == 0) return GNNMP_OK;                                     // no work: no HIP call, nothing written
    EpisodeDatasetStore st;
    st.n = s->n_problems; st.total_nodes = s->total_nodes; st.total_edges = s->total_edges; st.total_obs = s->total_obs;
    st.C = s->config_size; st.S = s->obs_size;
    st.v = s->v; st.points64 = s->points64; st.edge_index = reinterpret_cast<const long long*>(s->edge_index);
    st.edge_free = s->edge_free; st.edge_cost = s->edge_cost; st.obstacles = s->obstacles;
    st.node_ptr = s->node_ptr; st.edge_ptr = s->edge_ptr; st.obs_ptr = s->obs_ptr; st.status = s->status;
    EpisodeGatherParams p;
    p.G = n_group; p.total_nodes = out->total_nodes; p.total_edges = out->total_edges; p.total_obs = out->total_obs;
    p.idx = idx; p.v = out->v; p.points64 = out->points64; p.edge_index = reinterpret_cast<long long*>(out->edge_index);
    p.edge_free = out->edge_free; p.edge_cost = out->edge_cost; p.obstacles = out->obstacles;
    p.node_ptr = out->node_ptr; p.edge_ptr = out->edge_ptr; p.obs_ptr = out->obs_ptr;
    HIP_TRY(launch_episode_dataset_gather(st, p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_episode_frontier_loss(const gnnmp_episode_frontier_loss_desc* d, void* hip_stream) {
    if (!d) return GNNMP_ERR_NULL;
    if (d->n_problems < 0 || d->total_edges < 0 || !(d->divisor > 0.0) || !std::isfinite(d->divisor)) return GNNMP_ERR_ARG;
    if (!d->frontier || !d->frontier_len || !d->label || !d->status || !d->edge_ptr || !d->scores || !d->terms || !d->counted ||
        !d->loss || !d->dscores || !d->bad)
        return GNNMP_ERR_NULL;
    if (d->n_problems == 0) return GNNMP_OK;                               // no work: no HIP call, nothing written
    EpisodeFrontierLossParams p;
    p.B = d->n_problems; p.total_edges = d->total_edges; p.divisor = d->divisor;
    p.frontier = d->frontier; p.frontier_len = d->frontier_len; p.label = d->label; p.status = d->status;
    p.edge_ptr = d->edge_ptr; p.scores = d->scores; p.terms = d->terms; p.counted = d->counted; p.loss = d->loss;
    p.dscores = d->dscores; p.bad = d->bad;
    HIP_TRY(launch_episode_frontier_loss(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

// =============================================================================================
// the NEXT planning network of the arm families (next3d_kernels.hip; next_model/model3D.py:87-213)
// =============================================================================================
static bool next3d_dims_ok(int32_t dim, int32_t point_dim) { return dim >= 1 && dim <= 15 && (point_dim == 3 || point_dim == 6); }

extern "C" int gnnmp_next3d_weights_floats(int32_t dim, int32_t point_dim, size_t* n_floats) {
    if (!n_floats) return GNNMP_ERR_NULL;
    if (!next3d_dims_ok(dim, point_dim)) return GNNMP_ERR_DIMS;
    *n_floats = next3d_weights_floats();
    return GNNMP_OK;
}

extern "C" int gnnmp_next3d_workspace_bytes(int32_t n_problems, size_t* bytes) {
    if (!bytes) return GNNMP_ERR_NULL;
    if (n_problems < 0) return GNNMP_ERR_ARG;
    *bytes = next3d_workspace_bytes(n_problems);
    return GNNMP_OK;
}

extern "C" int gnnmp_next3d_pb_forward(const gnnmp_next3d_pb* d, void* hip_stream) {
    if (!d) return GNNMP_ERR_NULL;
    if (!next3d_dims_ok(d->dim, d->point_dim) || d->width != 15) return GNNMP_ERR_DIMS;
    if (d->n_problems < 0 || d->iters < 0) return GNNMP_ERR_ARG;
    if (d->workspace_bytes < next3d_workspace_bytes(d->n_problems) || reinterpret_cast<uintptr_t>(d->workspace) % 16) return GNNMP_ERR_ARG;
    if (!d->maps || !d->goals || !d->weights || !d->pb_rep || !d->workspace) return GNNMP_ERR_NULL;
    if (d->n_problems == 0) return GNNMP_OK;
    Next3dPbParams p;
    p.B = d->n_problems; p.dim = d->dim; p.pd = d->point_dim; p.iters = d->iters;
    p.maps = d->maps; p.goals = d->goals; p.weights = d->weights; p.pb_rep = d->pb_rep;
    p.workspace = static_cast<float*>(d->workspace);
    HIP_TRY(launch_next3d_pb_forward(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_next3d_state_forward(const gnnmp_next3d_states* d, void* hip_stream) {
    if (!d) return GNNMP_ERR_NULL;
    if (!next3d_dims_ok(d->dim, d->point_dim) || d->width != 15) return GNNMP_ERR_DIMS;
    if (d->n_states < 0 || d->n_problems < 0) return GNNMP_ERR_ARG;
    if (!d->inputs || !d->problem_of_state || !d->pb_rep || !d->weights || !d->y || !d->status) return GNNMP_ERR_NULL;
    if (d->n_states == 0) return GNNMP_OK;
    Next3dStateParams p;
    p.S = d->n_states; p.B = d->n_problems; p.dim = d->dim; p.pd = d->point_dim;
    p.inputs = d->inputs; p.problem_of_state = d->problem_of_state; p.pb_rep = d->pb_rep; p.weights = d->weights; p.y = d->y;
    p.status = d->status;
    HIP_TRY(launch_next3d_state_forward(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

// =============================================================================================
// training the 3-D NEXT network (next3d_train_kernels.hip).  The order of checks of the 2-D training entry points: the struct,
// dims, negative counts, NULL arrays, then the no-work return BEFORE ANY HIP CALL (it writes nothing), then the workspace.
// =============================================================================================
extern "C" int gnnmp_next3d_train_workspace_bytes(int32_t n_problems, int32_t iters, int32_t n_states, size_t* bytes) {
    if (!bytes) return GNNMP_ERR_NULL;
    if (n_problems < 0 || iters < 0 || n_states < 0) return GNNMP_ERR_ARG;
    Next3dTrainCarve c;
    next3d_train_carve(n_problems, iters, n_states, c);
    *bytes = c.total;
    return GNNMP_OK;
}

extern "C" int gnnmp_next3d_weights_t_floats(int32_t dim, int32_t point_dim, size_t* n_floats) {
    if (!n_floats) return GNNMP_ERR_NULL;
    if (!next3d_dims_ok(dim, point_dim)) return GNNMP_ERR_DIMS;
    *n_floats = next3d_weights_t_floats();
    return GNNMP_OK;
}

static int next3d_train_ws(int32_t B, int32_t iters, int32_t S, const void* ws, size_t ws_bytes, Next3dTrainCarve& c) {
    next3d_train_carve(B, iters, S, c);
    if (ws_bytes < c.total || (reinterpret_cast<uintptr_t>(ws) & 255)) return GNNMP_ERR_WORKSPACE;
    return GNNMP_OK;
}

extern "C" int gnnmp_next3d_train_forward(const gnnmp_next3d_train* d, void* hip_stream) {
    if (!d) return GNNMP_ERR_NULL;
    if (!next3d_dims_ok(d->dim, d->point_dim) || d->width != 15) return GNNMP_ERR_DIMS;
    if (d->n_problems < 0 || d->n_states < 0 || d->iters < 0) return GNNMP_ERR_ARG;
    if (!d->maps || !d->goals || !d->inputs || !d->problem_of_state || !d->weights || !d->pb_rep || !d->y || !d->status || !d->workspace)
        return GNNMP_ERR_NULL;
    if (d->n_problems == 0) return GNNMP_OK;                   // no work: no HIP call, nothing written
    Next3dTrainCarve c;
    if (int rc = next3d_train_ws(d->n_problems, d->iters, d->n_states, d->workspace, d->workspace_bytes, c)) return rc;
    Next3dPbParams p;
    p.B = d->n_problems; p.dim = d->dim; p.pd = d->point_dim; p.iters = d->iters;
    p.maps = d->maps; p.goals = d->goals; p.weights = d->weights; p.pb_rep = d->pb_rep; p.workspace = nullptr;
    Next3dStateParams q;
    q.S = d->n_states; q.B = d->n_problems; q.dim = d->dim; q.pd = d->point_dim;
    q.inputs = d->inputs; q.problem_of_state = d->problem_of_state; q.pb_rep = d->pb_rep; q.weights = d->weights; q.y = d->y;
    q.status = d->status;
    HIP_TRY(launch_next3d_train_forward(p, q, static_cast<char*>(d->workspace), c, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

static int next3d_train_bwd(const gnnmp_next3d_train_bwd* d, void* hip_stream, bool state_call) {
    if (!d) return GNNMP_ERR_NULL;
    if (!next3d_dims_ok(d->dim, d->point_dim) || d->width != 15) return GNNMP_ERR_DIMS;
    if (d->n_problems < 0 || d->n_states < 0 || d->iters < 0) return GNNMP_ERR_ARG;
    if (!d->goals || !d->inputs || !d->problem_of_state || !d->weights || !d->weights_t || !d->pb_rep || !d->dy || !d->dpb_rep ||
        !d->dweights || !d->workspace)
        return GNNMP_ERR_NULL;
    if (d->n_problems == 0 || (state_call && d->n_states == 0)) return GNNMP_OK;       // no work: no HIP call, nothing written
    Next3dTrainBwdParams p;
    if (int rc = next3d_train_ws(d->n_problems, d->iters, d->n_states, d->workspace, d->workspace_bytes, p.c)) return rc;
    p.B = d->n_problems; p.S = d->n_states; p.dim = d->dim; p.pd = d->point_dim; p.iters = d->iters;
    p.goals = d->goals; p.inputs = d->inputs; p.problem_of_state = d->problem_of_state; p.weights = d->weights;
    p.weights_t = d->weights_t; p.pb_rep = d->pb_rep; p.dy = d->dy; p.dpb_rep = d->dpb_rep; p.dweights = d->dweights;
    p.ws = static_cast<char*>(d->workspace);
    if (state_call) HIP_TRY(launch_next3d_state_backward(p, static_cast<hipStream_t>(hip_stream)));
    else HIP_TRY(launch_next3d_pb_backward(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_next3d_state_backward(const gnnmp_next3d_train_bwd* d, void* hip_stream) { return next3d_train_bwd(d, hip_stream, true); }
extern "C" int gnnmp_next3d_pb_backward(const gnnmp_next3d_train_bwd* d, void* hip_stream) { return next3d_train_bwd(d, hip_stream, false); }

// =============================================================================================
// NEXT's guided tree loop on maze problems (next_plan_kernels.hip; algorithm/tsa.py:12-81, 141-220)
// =============================================================================================
extern "C" int gnnmp_next_plan_max_nodes(void) { return next_plan_max_nodes(); }

extern "C" int gnnmp_next_plan(const gnnmp_next_plan_batch* b, const gnnmp_next_plan_tree* t, void* hip_stream) {
    if (!b || !t) return GNNMP_ERR_NULL;
    if (b->dim != 2 && b->dim != 3) return GNNMP_ERR_DIMS;
    if (b->width != 15) return GNNMP_ERR_DIMS;
    if (!b->maps || !b->init_states || !b->goal_states || !b->draws || !b->pb_rep || !b->weights || !b->eps) return GNNMP_ERR_NULL;
    if (!t->states || !t->parents || !t->rewired_parents || !t->flags || !t->costs || !t->path_lengths || !t->cumulated_checks ||
        !t->path || !t->n_nodes || !t->success || !t->last_iter || !t->used || !t->path_len || !t->status || !t->expanded_by_rrt ||
        !t->state_values || !t->w || !t->visits || !t->w_sum || !t->guided)
        return GNNMP_ERR_NULL;
    if (b->n_problems < 1 || b->t_max < 1 || (long long)b->t_max + 1 > next_plan_max_nodes()) return GNNMP_ERR_ARG;
    if (b->k < 1 || b->k > 16 || b->eps_rows < 1) return GNNMP_ERR_ARG;
    if (b->draws_per_problem < 2 + b->dim || b->draws_per_problem > INT32_MAX) return GNNMP_ERR_ARG;      // one iteration at least
    NextPlanParams p;
    p.t.B = b->n_problems; p.t.w = b->width; p.t.t_max = b->t_max; p.t.stop = b->stop_when_success ? 1 : 0; p.t.dim = b->dim;
    p.t.draw_len = b->draws_per_problem;
    p.t.maps = b->maps; p.t.init_states = b->init_states; p.t.goal_states = b->goal_states; p.t.draws = b->draws;
    p.t.states = t->states; p.t.parents = t->parents; p.t.rewired = t->rewired_parents; p.t.flags = t->flags; p.t.costs = t->costs;
    p.t.path_lengths = t->path_lengths; p.t.cum_checks = reinterpret_cast<long long*>(t->cumulated_checks); p.t.path = t->path;
    p.t.n_nodes = t->n_nodes; p.t.success = t->success; p.t.last_iter = t->last_iter; p.t.used = t->used; p.t.path_len = t->path_len;
    p.t.status = t->status;
    p.t.ws_x = p.t.ws_y = p.t.ws_z = p.t.ws_c = nullptr; p.t.ws_f = nullptr;
    p.g_explore_eps = b->g_explore_eps; p.c = b->c; p.k = b->k; p.eps_rows = b->eps_rows; p.scale = b->scale;
    p.pb_rep = b->pb_rep; p.weights = b->weights; p.eps = b->eps;
    p.by_rrt = t->expanded_by_rrt; p.state_values = t->state_values; p.w = t->w; p.visits = t->visits; p.w_sum = t->w_sum;
    p.guided = t->guided;
    HIP_TRY(launch_next_plan(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

// =============================================================================================
// training path of the explorer (train_explorer.py:156-186)
// =============================================================================================
namespace {

struct TrainCarve {
    size_t inf_bytes;                  // the inference workspace comes first (CSR, goal node, padded pointers stay valid)
    // offsets in floats from the start of the train region
    size_t NF, EF, NCin, NCh, NC, ECin, ECh, EC, H0, it0, it_stride, Xin, X, Zh, A, arg, H, DinCat, Dn, Pin, P1, P2, sc;
    size_t T5a, T5b, Te1, Te2, T3, dX, dH, dA, dNC, dH0, dXin, dEC, cat2, dcat2, dDn;
    size_t obeg, ocnt, ocur, oslot;    // edges grouped by source (ints), built by the forward, read by the backward
    size_t dwp;                        // per-block partial sums of the weight gradients (two-stage, deterministic)
    size_t total_floats;
};

bool train_carve(const gnnmp_explorer* h, const gnnmp_batch* b, int loop, const Carve& c, TrainCarve& t) {
    const size_t Np = c.Npad, Ep = c.Epad, d = h->dims.embed_size, C = h->dims.config_size;
    size_t o = 0;
    auto take = [&](size_t n) { const size_t r = o; o += (n + 63) & ~(size_t)63; return r; };
    t.inf_bytes = (c.total + 255) & ~(size_t)255;
    t.NF = take(Np * d); t.EF = take(Ep * d);
    t.NCin = take(Np * 4 * C); t.NCh = take(Np * d); t.NC = take(Np * d);
    t.ECin = take(Ep * 2 * C); t.ECh = take(Ep * d); t.EC = take(Ep * d);
    t.H0 = take(Np * d);
    t.it0 = o;
    t.Xin = take(Np * 4 * d) - t.it0; t.X = take(Np * d) - t.it0; t.Zh = take(Ep * d) - t.it0; t.A = take(Np * d) - t.it0;
    t.arg = take(Np * d) - t.it0; t.H = take(Np * d) - t.it0;
    t.it_stride = o - t.it0;
    o = t.it0 + t.it_stride * (size_t)loop;
    t.DinCat = take(Np * 2 * d); t.Dn = take(Np * d);
    t.Pin = take(Ep * 3 * d); t.P1 = take(Ep * d); t.P2 = take(Ep * d); t.sc = take(Ep);
    t.T5a = take(Ep * 5 * d); t.T5b = take(Ep * 5 * d); t.Te1 = take(Ep * d); t.Te2 = take(Ep * d); t.T3 = take(Ep * 3 * d);
    t.dX = take(Np * d); t.dH = take(Np * d); t.dA = take(Np * d); t.dNC = take(Np * d); t.dH0 = take(Np * d);
    t.dXin = take(Np * 4 * d); t.dEC = take(Ep * d); t.cat2 = take(Np * 2 * d); t.dcat2 = take(Np * 2 * d); t.dDn = take(Np * d);
    t.obeg = take(Np); t.ocnt = take(Np); t.ocur = take(Np); t.oslot = take(Ep);
    {
        size_t m = t_linear_dw_scratch_floats((int)Ep, (int)(5 * d), (int)d);          // the widest layer over edge rows ...
        const size_t n4 = t_linear_dw_scratch_floats((int)Np, (int)(4 * d), (int)d);  // ... and over node rows
        t.dwp = take(m > n4 ? m : n4);
    }
    t.total_floats = o;
    (void)b;
    return true;
}

struct WRef { const float* w; const float* b; float* gw; float* gb; int out, in; };

// weight / bias of a Linear named `name` inside the raw blob, and the same slots inside the gradient blob
WRef wref(const gnnmp_explorer* h, float* grad, const std::string& name, bool bias = true) {
    WRef r{nullptr, nullptr, nullptr, nullptr, 0, 0};
    for (size_t i = 0; i < h->man.size(); ++i) {
        if (h->man[i].name == name + ".weight") {
            r.w = h->w_raw_dev + h->man_off[i]; r.gw = grad ? grad + h->man_off[i] : nullptr;
            r.out = h->man[i].rows; r.in = h->man[i].cols;
        }
        if (bias && h->man[i].name == name + ".bias") { r.b = h->w_raw_dev + h->man_off[i]; r.gb = grad ? grad + h->man_off[i] : nullptr; }
    }
    return r;
}

TrainGeom train_geom(const gnnmp_explorer* h, const gnnmp_batch* b, const Carve& c, const TrainCarve& t, void* ws) {
    TrainGeom q;
    q.G = c.G; q.C = h->dims.config_size; q.Npad = c.Npad; q.Epad = c.Epad;
    q.v = b->v; q.goal = b->goal; q.node_ptr = b->node_ptr;
    q.node_ptr_pad = at<int>(ws, c.node_ptr_pad); q.ntile_graph = at<int>(ws, c.ntile_graph);
    q.goal_node = at<int>(ws, c.goal_node); q.row_beg = at<int>(ws, c.row_beg); q.deg = at<int>(ws, c.deg);
    q.csr = at<int4>(ws, c.csr);
    int* TI = reinterpret_cast<int*>(static_cast<char*>(ws) + t.inf_bytes);
    q.out_beg = TI + t.obeg; q.out_cnt = TI + t.ocnt; q.out_cur = TI + t.ocur; q.out_slot = TI + t.oslot;
    return q;
}

TrainGeom geom_prefix(TrainGeom q, int Np, int Ep) {      // the geometry launchers bound their rows / slots by these two
    q.Npad = Np; q.Epad = Ep;
    return q;
}

// the Linears of the training path inside the raw blob, and (grad != nullptr) their slots inside the gradient blob
struct TrainWeights {
    WRef nc0, nc2, ec0, ec2, enc, l00, l02, l1, dec, p0, p2, p4;
    const float* ge;                   // goal_encoder
    float* g_ge;
};

TrainWeights train_weights(const gnnmp_explorer* h, float* grad) {
    TrainWeights w{wref(h, grad, "node_code.0"), wref(h, grad, "node_code.2"), wref(h, grad, "edge_code.0"), wref(h, grad, "edge_code.2"),
                   wref(h, grad, "encoder"), wref(h, grad, "process.lin_0.0"), wref(h, grad, "process.lin_0.2"),
                   wref(h, grad, "process.lin_1"), wref(h, grad, "decoder"), wref(h, grad, "policy.0"), wref(h, grad, "policy.2"),
                   wref(h, grad, "policy.4", false), nullptr, nullptr};
    for (size_t i = 0; i < h->man.size(); ++i)
        if (h->man[i].name == "goal_encoder") { w.ge = h->w_raw_dev + h->man_off[i]; w.g_ge = grad ? grad + h->man_off[i] : nullptr; }
    return w;
}

// the rows each iteration covers.  Batched call (a loop count per graph, longest first): the graphs of iteration `it` are a prefix of
// the padded node / edge space, gnnmp_explorer_train_batch_plan.  Uniform call: no host-side counts and no bound on L, so every
// iteration covers the upper bounds No / Eo and the tables stay unused
struct TrainPlan {
    int L;                                               // iterations: loop, or loops_host[0]
    bool uniform;
    int No, Eo;                                          // c.Npad / c.Epad: t_linear_dw's R_order (train_setup fills them)
    int A[kTrainBatchMaxLoop], Npi[kTrainBatchMaxLoop], Epi[kTrainBatchMaxLoop];
    int Np(int it) const { return uniform ? No : Npi[it]; }
    int Ep(int it) const { return uniform ? Eo : Epi[it]; }
};

struct TrainSetup { Carve c; TrainCarve t; float* T; };

// what the four entry points do after their own argument checks: carve, check the workspace, find the train region
int train_setup(const gnnmp_explorer* h, const gnnmp_batch* b, void* ws, size_t ws_bytes, TrainPlan& pl, TrainSetup& s) {
    if (!carve(h, b, s.c)) return GNNMP_ERR_ARG;
    train_carve(h, b, pl.L, s.c, s.t);
    if (ws_bytes < s.t.inf_bytes + s.t.total_floats * sizeof(float) || (reinterpret_cast<uintptr_t>(ws) & 255)) return GNNMP_ERR_WORKSPACE;
    s.T = reinterpret_cast<float*>(static_cast<char*>(ws) + s.t.inf_bytes);
    pl.No = s.c.Npad; pl.Eo = s.c.Epad;
    return GNNMP_OK;
}

// ---- one forward and one backward for both calls.  On a uniform plan every prefix is the whole padded space and t_seed_dh /
// R_order move the values the plain split / slice order would: the bits are those of a body written for one loop count
int explorer_train_forward_body(const gnnmp_explorer* h, const gnnmp_batch* b, const TrainPlan& pl, const TrainSetup& s,
                                int use_obstacles, float* edge_scores, void* ws, void* hip_stream) {
    const TrainCarve& t = s.t;
    float* T = s.T;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int d = h->dims.embed_size, C = h->dims.config_size;
    const int Np = pl.Np(0), Ep = pl.Ep(0);             // every graph runs iteration 0: the rows in use (<= No / Eo, upper bounds)
    // rows no kernel writes (padding tiles, graphs past their loop count) must hold finite numbers: the weight gradients sum
    // 0 * activation over them
    HIP_TRY(hipMemsetAsync(T, 0, t.total_floats * sizeof(float), st));
    // frozen inputs (model.py:141,142,146 detach them): node_free_code / edge_free_code after the attention stacks
    const int rc = forward_impl(h, b, pl.L, use_obstacles, nullptr, nullptr, ws, t.inf_bytes, hip_stream, T + t.NF, T + t.EF, true);
    if (rc != GNNMP_OK) return rc;
    const TrainGeom q = train_geom(h, b, s.c, t, ws);
    const TrainGeom qa = geom_prefix(q, Np, Ep);
    const TrainWeights w = train_weights(h, nullptr);
    HIP_TRY(t_out_csr(q, st));                                   // edges by source: the backward's gather adjoints walk it in order
    HIP_TRY(t_node_in(qa, T + t.NCin, st));
    HIP_TRY(t_linear(Np, 4 * C, d, T + t.NCin, w.nc0.w, w.nc0.b, T + t.NCh, true, st));
    HIP_TRY(t_linear(Np, d, d, T + t.NCh, w.nc2.w, w.nc2.b, T + t.NC, false, st));
    HIP_TRY(t_edge_in(qa, T + t.ECin, st));
    HIP_TRY(t_linear(Ep, 2 * C, d, T + t.ECin, w.ec0.w, w.ec0.b, T + t.ECh, true, st));
    HIP_TRY(t_linear(Ep, d, d, T + t.ECh, w.ec2.w, w.ec2.b, T + t.EC, false, st));
    HIP_TRY(t_h0(qa, d, w.ge, T + t.H0, st));
    const float* Hprev = T + t.H0;
    for (int it = 0; it < pl.L; ++it) {
        float* I = T + t.it0 + t.it_stride * (size_t)it;
        const int Na = pl.Np(it), Ea = pl.Ep(it);        // graphs with loops_host[g] > it
        const TrainGeom qi = geom_prefix(q, Na, Ea);
        HIP_TRY(t_concat(Na, d, 4, T + t.NC, T + t.NF, T + t.H0, Hprev, I + t.Xin, st));                 // model.py:141
        HIP_TRY(t_linear(Na, 4 * d, d, I + t.Xin, w.enc.w, w.enc.b, I + t.X, false, st));
        HIP_TRY(t_msg_in(qi, d, I + t.X, T + t.EF, T + t.EC, T + t.T5a, st));                            // model.py:38-39
        HIP_TRY(t_linear(Ea, 5 * d, d, T + t.T5a, w.l00.w, w.l00.b, I + t.Zh, true, st));
        HIP_TRY(t_linear(Ea, d, d, I + t.Zh, w.l02.w, w.l02.b, T + t.Te1, false, st));
        HIP_TRY(t_segment_max(qi, d, T + t.Te1, I + t.A, reinterpret_cast<int*>(I + t.arg), st));        // model.py:33
        HIP_TRY(t_concat(Na, d, 2, I + t.X, I + t.A, nullptr, nullptr, T + t.cat2, st));
        HIP_TRY(t_linear(Na, 2 * d, d, T + t.cat2, w.l1.w, w.l1.b, I + t.H, false, st));                 // model.py:36
        Hprev = I + t.H;
    }
    // every graph's own last hidden state (model.py:143 at loop = loops_host[g]); one loop count: the last iteration's, whatever L is
    if (pl.uniform) {
        HIP_TRY(t_concat(Np, d, 2, T + t.NC, Hprev, nullptr, nullptr, T + t.DinCat, st));
    } else {
        TrainLoopRows lr;
        lr.n_it = pl.L;
        for (int it = 0; it < kTrainBatchMaxLoop; ++it) lr.rows[it] = it < pl.L ? pl.Npi[it] : 0;
        HIP_TRY(t_final_cat(lr, d, T + t.NC, T + t.it0 + t.H, t.it_stride, T + t.DinCat, st));
    }
    HIP_TRY(t_linear(Np, 2 * d, d, T + t.DinCat, w.dec.w, w.dec.b, T + t.Dn, false, st));
    HIP_TRY(t_pol_in(qa, d, T + t.Dn, T + t.EF, T + t.Pin, st));                                         // model.py:145
    HIP_TRY(t_linear(Ep, 3 * d, d, T + t.Pin, w.p0.w, w.p0.b, T + t.P1, true, st));
    HIP_TRY(t_linear(Ep, d, d, T + t.P1, w.p2.w, w.p2.b, T + t.P2, true, st));
    HIP_TRY(t_linear(Ep, d, 1, T + t.P2, w.p4.w, nullptr, T + t.sc, false, st));
    if (b->total_edges > 0) HIP_TRY(t_scores_out(qa, T + t.sc, edge_scores, st));
    return GNNMP_OK;
}

int explorer_train_backward_body(const gnnmp_explorer* h, const gnnmp_batch* b, const TrainPlan& pl, const TrainSetup& s,
                                 const float* d_edge_scores, float* grad, void* ws, void* hip_stream) {
    const TrainCarve& t = s.t;
    float* T = s.T;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int d = h->dims.embed_size, C = h->dims.config_size;
    const int Np = pl.Np(0), Ep = pl.Ep(0);
    // the weight gradients' second stage sums in the order of a call over No / Eo rows (the missing ones all zero)
    const int No = pl.No, Eo = pl.Eo;
    const TrainGeom q = train_geom(h, b, s.c, t, ws);
    const TrainGeom qa = geom_prefix(q, Np, Ep);
    HIP_TRY(hipMemsetAsync(grad, 0, (size_t)h->n_raw * sizeof(float), st));
    const TrainWeights w = train_weights(h, grad);
    // ---- policy head (model.py:145-146), all graphs
    HIP_TRY(t_scores_in(qa, d_edge_scores, T + t.Te1, st));                         // [Ep, 1]
    HIP_TRY(t_linear_dw(Ep, d, 1, T + t.Te1, T + t.P2, w.p4.gw, nullptr, T + t.dwp, st, Eo));
    HIP_TRY(t_linear_dx(Ep, d, 1, T + t.Te1, w.p4.w, T + t.Te2, false, st));        // dP2
    HIP_TRY(t_relu_bwd((size_t)Ep * d, T + t.P2, T + t.Te2, st));
    HIP_TRY(t_linear_dw(Ep, d, d, T + t.Te2, T + t.P1, w.p2.gw, w.p2.gb, T + t.dwp, st, Eo));
    HIP_TRY(t_linear_dx(Ep, d, d, T + t.Te2, w.p2.w, T + t.Te1, false, st));        // dP1
    HIP_TRY(t_relu_bwd((size_t)Ep * d, T + t.P1, T + t.Te1, st));
    HIP_TRY(t_linear_dw(Ep, 3 * d, d, T + t.Te1, T + t.Pin, w.p0.gw, w.p0.gb, T + t.dwp, st, Eo));
    HIP_TRY(t_linear_dx(Ep, 3 * d, d, T + t.Te1, w.p0.w, T + t.T3, false, st));     // dPin
    HIP_TRY(t_fill((size_t)Np * d, T + t.dDn, 0.f, st));
    HIP_TRY(t_pol_in_bwd(qa, d, T + t.T3, T + t.dDn, st));
    // ---- decoder (model.py:143): its input gradient's second half is d h_final of EVERY graph; it waits in dDn (free from here on)
    // until the backward loop reaches the graph's last iteration
    HIP_TRY(t_linear_dw(Np, 2 * d, d, T + t.dDn, T + t.DinCat, w.dec.gw, w.dec.gb, T + t.dwp, st, No));
    HIP_TRY(t_linear_dx(Np, 2 * d, d, T + t.dDn, w.dec.w, T + t.dcat2, false, st));
    HIP_TRY(t_split(Np, d, 2, 0, T + t.dcat2, T + t.dNC, false, st));
    HIP_TRY(t_split(Np, d, 2, 1, T + t.dcat2, T + t.dDn, false, st));
    HIP_TRY(t_fill((size_t)Np * d, T + t.dH0, 0.f, st));
    HIP_TRY(t_fill((size_t)Ep * d, T + t.dEC, 0.f, st));
    // ---- the loop, backwards (model.py:139-142), iteration `it` over the graphs that ran it
    for (int it = pl.L - 1; it >= 0; --it) {
        float* I = T + t.it0 + t.it_stride * (size_t)it;
        const int Na = pl.Np(it), Ea = pl.Ep(it);
        const TrainGeom qi = geom_prefix(q, Na, Ea);
        HIP_TRY(t_seed_dh(Na, it + 1 < pl.L ? pl.Np(it + 1) : 0, d, T + t.dDn, T + t.dXin, T + t.dH, st));
        HIP_TRY(t_concat(Na, d, 2, I + t.X, I + t.A, nullptr, nullptr, T + t.cat2, st));
        HIP_TRY(t_linear_dw(Na, 2 * d, d, T + t.dH, T + t.cat2, w.l1.gw, w.l1.gb, T + t.dwp, st, No));
        HIP_TRY(t_linear_dx(Na, 2 * d, d, T + t.dH, w.l1.w, T + t.dcat2, false, st));
        HIP_TRY(t_split(Na, d, 2, 0, T + t.dcat2, T + t.dX, false, st));
        HIP_TRY(t_split(Na, d, 2, 1, T + t.dcat2, T + t.dA, false, st));
        HIP_TRY(t_fill((size_t)Ea * d, T + t.Te1, 0.f, st));                        // dM
        HIP_TRY(t_segment_max_bwd(Na, d, T + t.dA, reinterpret_cast<const int*>(I + t.arg), T + t.Te1, st));
        HIP_TRY(t_linear_dw(Ea, d, d, T + t.Te1, I + t.Zh, w.l02.gw, w.l02.gb, T + t.dwp, st, Eo));
        HIP_TRY(t_linear_dx(Ea, d, d, T + t.Te1, w.l02.w, T + t.Te2, false, st));    // dZh
        HIP_TRY(t_relu_bwd((size_t)Ea * d, I + t.Zh, T + t.Te2, st));
        HIP_TRY(t_msg_in(qi, d, I + t.X, T + t.EF, T + t.EC, T + t.T5a, st));        // Zin recomputed
        HIP_TRY(t_linear_dw(Ea, 5 * d, d, T + t.Te2, T + t.T5a, w.l00.gw, w.l00.gb, T + t.dwp, st, Eo));
        HIP_TRY(t_linear_dx(Ea, 5 * d, d, T + t.Te2, w.l00.w, T + t.T5b, false, st)); // dZin
        HIP_TRY(t_msg_in_bwd(qi, d, T + t.T5b, T + t.dX, T + t.dEC, st));
        HIP_TRY(t_linear_dw(Na, 4 * d, d, T + t.dX, I + t.Xin, w.enc.gw, w.enc.gb, T + t.dwp, st, No));
        HIP_TRY(t_linear_dx(Na, 4 * d, d, T + t.dX, w.enc.w, T + t.dXin, false, st));
        HIP_TRY(t_split(Na, d, 4, 0, T + t.dXin, T + t.dNC, true, st));              // node_code
        HIP_TRY(t_split(Na, d, 4, 2, T + t.dXin, T + t.dH0, true, st));              // h_0   (part 1 = node_free_code: detached)
        // part 3, d h_{i-1}: the next round's t_seed_dh takes it; h_i of the first iteration IS h_0
        if (it == 0) HIP_TRY(t_split(Na, d, 4, 3, T + t.dXin, T + t.dH0, true, st));
    }
    HIP_TRY(t_h0_bwd(qa, d, T + t.dH0, w.g_ge, st));
    // ---- edge_code, node_code encoders (model.py:119-120), all graphs
    HIP_TRY(t_linear_dw(Ep, d, d, T + t.dEC, T + t.ECh, w.ec2.gw, w.ec2.gb, T + t.dwp, st, Eo));
    HIP_TRY(t_linear_dx(Ep, d, d, T + t.dEC, w.ec2.w, T + t.Te1, false, st));
    HIP_TRY(t_relu_bwd((size_t)Ep * d, T + t.ECh, T + t.Te1, st));
    HIP_TRY(t_linear_dw(Ep, 2 * C, d, T + t.Te1, T + t.ECin, w.ec0.gw, w.ec0.gb, T + t.dwp, st, Eo));
    HIP_TRY(t_linear_dw(Np, d, d, T + t.dNC, T + t.NCh, w.nc2.gw, w.nc2.gb, T + t.dwp, st, No));
    HIP_TRY(t_linear_dx(Np, d, d, T + t.dNC, w.nc2.w, T + t.dX, false, st));
    HIP_TRY(t_relu_bwd((size_t)Np * d, T + t.NCh, T + t.dX, st));
    HIP_TRY(t_linear_dw(Np, 4 * C, d, T + t.dX, T + t.NCin, w.nc0.gw, w.nc0.gb, T + t.dwp, st, No));
    return GNNMP_OK;
}

}  // namespace

extern "C" int64_t gnnmp_explorer_grad_floats(const gnnmp_explorer* h) { return h ? h->n_raw : GNNMP_ERR_NULL; }

extern "C" int gnnmp_explorer_train_workspace_bytes(const gnnmp_explorer* h, const gnnmp_batch* shape, int loop, size_t* bytes) {
    if (!h || !shape || !bytes) return GNNMP_ERR_NULL;
    if (loop < 1) return GNNMP_ERR_ARG;
    if (h->dims.mlp_dtype != GNNMP_F32) return GNNMP_ERR_DIMS;          // training runs in fp32
    Carve c;
    if (!carve(h, shape, c)) return GNNMP_ERR_ARG;
    TrainCarve t;
    train_carve(h, shape, loop, c, t);
    *bytes = t.inf_bytes + t.total_floats * sizeof(float);
    return GNNMP_OK;
}

extern "C" int gnnmp_explorer_train_forward(const gnnmp_explorer* h, const gnnmp_batch* b, int loop, int use_obstacles,
                                            float* edge_scores, void* ws, size_t ws_bytes, void* hip_stream) {
    if (!h || !b || !ws || (b->total_edges > 0 && !edge_scores)) return GNNMP_ERR_NULL;
    if (!b->node_ptr || !b->edge_ptr || !b->obs_ptr) return GNNMP_ERR_NULL;     // the training path takes explicit prefix arrays
    if (loop < 1) return GNNMP_ERR_ARG;
    if (h->dims.mlp_dtype != GNNMP_F32) return GNNMP_ERR_DIMS;
    TrainPlan pl;
    pl.L = loop; pl.uniform = true;
    TrainSetup s;
    const int rc = train_setup(h, b, ws, ws_bytes, pl, s);
    return rc != GNNMP_OK ? rc : explorer_train_forward_body(h, b, pl, s, use_obstacles, edge_scores, ws, hip_stream);
}

extern "C" int gnnmp_explorer_train_backward(const gnnmp_explorer* h, const gnnmp_batch* b, int loop, const float* d_edge_scores,
                                             float* grad, void* ws, size_t ws_bytes, void* hip_stream) {
    if (!h || !b || !ws || !grad || (b->total_edges > 0 && !d_edge_scores)) return GNNMP_ERR_NULL;
    if (!b->node_ptr || !b->edge_ptr || !b->obs_ptr) return GNNMP_ERR_NULL;
    if (loop < 1) return GNNMP_ERR_ARG;
    if (h->dims.mlp_dtype != GNNMP_F32) return GNNMP_ERR_DIMS;           // same argument checks as train_forward
    TrainPlan pl;
    pl.L = loop; pl.uniform = true;
    TrainSetup s;
    const int rc = train_setup(h, b, ws, ws_bytes, pl, s);
    return rc != GNNMP_OK ? rc : explorer_train_backward_body(h, b, pl, s, d_edge_scores, grad, ws, hip_stream);
}

// ---- a loop count per graph (train_explorer.py:148), graphs longest loop first: the graphs of iteration `it` are a prefix of the
// batch, of the padded node space and of the padded CSR edge space, and every launch of that iteration covers the prefix only
extern "C" int gnnmp_explorer_train_batch_plan(int32_t n_graphs, const int32_t* loops_host, const int32_t* node_counts_host,
                                               const int32_t* edge_counts_host, int32_t cap, int32_t* active, int32_t* node_rows,
                                               int32_t* edge_rows, int32_t* n_iters) {
    if (!loops_host || !node_counts_host || !edge_counts_host || !n_iters) return GNNMP_ERR_NULL;
    if (cap > 0 && (!active || !node_rows || !edge_rows)) return GNNMP_ERR_NULL;
    if (n_graphs < 1 || cap < 0) return GNNMP_ERR_ARG;
    for (int g = 0; g < n_graphs; ++g) {
        if (loops_host[g] < 1 || loops_host[g] > GNNMP_TRAIN_BATCH_MAX_LOOP) return GNNMP_ERR_ARG;
        if (g > 0 && loops_host[g] > loops_host[g - 1]) return GNNMP_ERR_ARG;          // longest first
        if (node_counts_host[g] < 0 || edge_counts_host[g] < 0) return GNNMP_ERR_ARG;
    }
    *n_iters = loops_host[0];
    if (cap == 0) return GNNMP_OK;
    if (cap < loops_host[0]) return GNNMP_ERR_ARG;
    // iterations from the last to the first: the prefix only grows, so one walk over the graphs serves all of them
    int a = 0;
    long long nr = 0, er = 0;
    for (int it = loops_host[0] - 1; it >= 0; --it) {
        while (a < n_graphs && loops_host[a] > it) {
            nr += round_up_i(node_counts_host[a], kPad);           // the prep stage's rule (prep_prefix): node_ptr_pad / edge_ptr_pad
            er += round_up_i(edge_counts_host[a], kPad);
            ++a;
        }
        if (nr > 0x7fffffffLL || er > 0x7fffffffLL) return GNNMP_ERR_ARG;
        active[it] = a; node_rows[it] = (int)nr; edge_rows[it] = (int)er;
    }
    return GNNMP_OK;
}

namespace {

// the argument checks the three entry points share; GNNMP_OK and the plan
int train_batch_args(const gnnmp_explorer* h, const gnnmp_batch* b, const int32_t* loops, const int32_t* ncnt, const int32_t* ecnt,
                     TrainPlan& p) {
    p.uniform = false;
    const int rc = gnnmp_explorer_train_batch_plan(b->n_graphs, loops, ncnt, ecnt, kTrainBatchMaxLoop, p.A, p.Npi, p.Epi, &p.L);
    if (rc != GNNMP_OK) return rc;
    long long n = 0, e = 0;
    for (int g = 0; g < b->n_graphs; ++g) { n += ncnt[g]; e += ecnt[g]; }
    if (n != b->total_nodes || e != b->total_edges) return GNNMP_ERR_ARG;
    if (h->dims.mlp_dtype != GNNMP_F32) return GNNMP_ERR_DIMS;          // training runs in fp32
    return GNNMP_OK;
}

}  // namespace

extern "C" int gnnmp_explorer_train_batch_workspace_bytes(const gnnmp_explorer* h, const gnnmp_batch* shape, const int32_t* loops_host,
                                                          const int32_t* node_counts_host, const int32_t* edge_counts_host,
                                                          size_t* bytes) {
    if (!h || !shape || !loops_host || !node_counts_host || !edge_counts_host || !bytes) return GNNMP_ERR_NULL;
    TrainPlan p;
    const int rc = train_batch_args(h, shape, loops_host, node_counts_host, edge_counts_host, p);
    if (rc != GNNMP_OK) return rc;
    return gnnmp_explorer_train_workspace_bytes(h, shape, p.L, bytes);
}

extern "C" int gnnmp_explorer_train_batch_forward(const gnnmp_explorer* h, const gnnmp_batch* b, const int32_t* loops_host,
                                                  const int32_t* node_counts_host, const int32_t* edge_counts_host, int use_obstacles,
                                                  float* edge_scores, void* ws, size_t ws_bytes, void* hip_stream) {
    if (!h || !b || !loops_host || !node_counts_host || !edge_counts_host || !ws || (b->total_edges > 0 && !edge_scores))
        return GNNMP_ERR_NULL;
    if (!b->node_ptr || !b->edge_ptr || !b->obs_ptr) return GNNMP_ERR_NULL;
    TrainPlan pl;
    TrainSetup s;
    int rc = train_batch_args(h, b, loops_host, node_counts_host, edge_counts_host, pl);
    if (rc == GNNMP_OK) rc = train_setup(h, b, ws, ws_bytes, pl, s);
    return rc != GNNMP_OK ? rc : explorer_train_forward_body(h, b, pl, s, use_obstacles, edge_scores, ws, hip_stream);
}

extern "C" int gnnmp_explorer_train_batch_backward(const gnnmp_explorer* h, const gnnmp_batch* b, const int32_t* loops_host,
                                                   const int32_t* node_counts_host, const int32_t* edge_counts_host,
                                                   const float* d_edge_scores, float* grad, void* ws, size_t ws_bytes, void* hip_stream) {
    if (!h || !b || !loops_host || !node_counts_host || !edge_counts_host || !ws || !grad || (b->total_edges > 0 && !d_edge_scores))
        return GNNMP_ERR_NULL;
    if (!b->node_ptr || !b->edge_ptr || !b->obs_ptr) return GNNMP_ERR_NULL;
    TrainPlan pl;
    TrainSetup s;
    int rc = train_batch_args(h, b, loops_host, node_counts_host, edge_counts_host, pl);
    if (rc == GNNMP_OK) rc = train_setup(h, b, ws, ws_bytes, pl, s);
    return rc != GNNMP_OK ? rc : explorer_train_backward_body(h, b, pl, s, d_edge_scores, grad, ws, hip_stream);
}

// =============================================================================================
// training path of the smoother (train_smoother.py:33-61; model_smoother.py:104-142 under model.train())
// =============================================================================================
namespace {

struct SmTrainCarve {
    size_t inf_bytes;
    int Nn, K0, ecap;
    // floats from the start of the train region
    size_t states, it0, it_stride, Xin, X0, stats, X1, X, esrc, edst, ne, Zh, S, L1h, Hh;
    size_t Zin, M, dZh, dZin, dX, dX1, dX0, dXin, dS, dL1h, dHh, prop, dprop, dpa, dpb, tmpP, dwp;
    size_t total_floats;
};

// for B = b->n_problems problems (the per-problem calls: B = 1, sm_train_ok): per iteration, stats [B][3][d] and edge counts [B]
bool sm_train_carve(const gnnmp_smoother* h, const gnnmp_smooth_batch* b, int loop, const SmCarve& c, SmTrainCarve& t) {
    const size_t d = h->dims.embed_size, C = h->dims.config_size, P = b->total_path, B = b->n_problems;
    t.Nn = b->total_path + b->total_free + b->total_collided;
    t.K0 = (int)C + 3;
    t.ecap = c.ecap;
    const size_t Nn = t.Nn, Ec = t.ecap, K0 = t.K0;
    size_t o = 0;
    auto take = [&](size_t n) { const size_t r = o; o += (n + 63) & ~(size_t)63; return r; };
    t.inf_bytes = (c.total + 255) & ~(size_t)255;
    t.states = take((size_t)(loop + 1) * P * C);
    t.it0 = o;
    t.Xin = take(Nn * K0) - t.it0; t.X0 = take(Nn * d) - t.it0; t.stats = take(B * 3 * d) - t.it0; t.X1 = take(Nn * d) - t.it0;
    t.X = take(Nn * d) - t.it0; t.esrc = take(Ec) - t.it0; t.edst = take(Ec) - t.it0; t.ne = take(B) - t.it0;
    t.Zh = take(Ec * d) - t.it0; t.S = take(P * d) - t.it0; t.L1h = take(P * d) - t.it0; t.Hh = take(P * d) - t.it0;
    t.it_stride = o - t.it0;
    o = t.it0 + t.it_stride * (size_t)(loop > 0 ? loop : 1);
    t.Zin = take(Ec * 3 * d); t.M = take(Ec * d); t.dZh = take(Ec * d); t.dZin = take(Ec * 3 * d);
    t.dX = take(Nn * d); t.dX1 = take(Nn * d); t.dX0 = take(Nn * d); t.dXin = take(Nn * K0);
    t.dS = take(P * d); t.dL1h = take(P * d); t.dHh = take(P * d); t.prop = take(P * C); t.dprop = take(P * C);
    t.dpa = take(P * C); t.dpb = take(P * C); t.tmpP = take(P * d);
    {
        size_t m = t_linear_dw_scratch_floats((int)Ec, (int)(3 * d), (int)d);
        const size_t n1 = t_linear_dw_scratch_floats((int)Nn, (int)d, (int)d), n0 = t_linear_dw_scratch_floats((int)Nn, (int)K0, (int)d);
        m = m > n1 ? m : n1;
        t.dwp = take(m > n0 ? m : n0);
    }
    t.total_floats = o;
    return true;
}

struct SmW { const float* w; const float* b; float* gw; float* gb; };
SmW sm_wref(const gnnmp_smoother* h, float* grad, const std::string& name) {
    SmW r{nullptr, nullptr, nullptr, nullptr};
    for (size_t i = 0; i < h->man.size(); ++i) {
        if (h->man[i].name == name + ".weight") { r.w = h->w_raw_dev + h->man_off[i]; r.gw = grad ? grad + h->man_off[i] : nullptr; }
        if (h->man[i].name == name + ".bias") { r.b = h->w_raw_dev + h->man_off[i]; r.gb = grad ? grad + h->man_off[i] : nullptr; }
    }
    return r;
}
struct SmWeights { SmW nc0, bn, nc3, l00, l02, l10, l12, sn; };
SmWeights sm_weights(const gnnmp_smoother* h, float* grad) {
    return {sm_wref(h, grad, "node_code.0"), sm_wref(h, grad, "node_code.1"), sm_wref(h, grad, "node_code.3"),
            sm_wref(h, grad, "process.lin_0.0"), sm_wref(h, grad, "process.lin_0.2"), sm_wref(h, grad, "process.lin_1.0"),
            sm_wref(h, grad, "process.lin_1.2"), sm_wref(h, grad, "smooth_node")};
}

bool sm_train_ok(const gnnmp_smoother* h, const gnnmp_smooth_batch* b) {
    return b->path_ptr && b->free_ptr && b->coll_ptr && b->edge_ptr && b->n_problems == 1 && b->total_path >= 1 && h->dims.mlp_dtype == GNNMP_F32 && b->max_samples <= 2048;
}

void sm_fill_params(const gnnmp_smoother* h, const gnnmp_smooth_batch* b, const SmCarve& c, void* ws, SmParams& p) {
    p.B = 1; p.C = h->dims.config_size; p.total_path = b->total_path; p.total_edges = b->total_edges;
    p.scale = h->dims.scale;
    p.path = b->path; p.free_pts = b->free_pts; p.collided = b->collided;
    p.edge_index = reinterpret_cast<const long long*>(b->edge_index);
    p.path_ptr = b->path_ptr; p.free_ptr = b->free_ptr; p.coll_ptr = b->coll_ptr; p.edge_ptr = b->edge_ptr;
    p.w = h->w_dev; p.L = h->L;
    p.knn = at<int>(ws, c.knn);
    p.e_src = at<int>(ws, c.e_src); p.e_dst = at<int>(ws, c.e_dst); p.e_count = at<int>(ws, c.e_count);
    p.stat = at<int>(ws, c.stat);
    p.seg_beg = at<int>(ws, c.seg_beg); p.seg_cnt = at<int>(ws, c.seg_cnt);
    p.etile_prob = at<int>(ws, c.etile); p.ptile_prob = at<int>(ws, c.ptile);
    p.msg = at<float>(ws, c.msg);
    p.tgt = at<float>(ws, c.tgt); p.tgt_flag = at<int>(ws, c.tflag);
    p.tile_cnt = nullptr; p.elist = nullptr; p.plist = nullptr; p.parity = 0;      // training path: no tile lists (its kernels walk the padded tile space)
    { static const int no_tgt = getenv("GNNMP_SM_NO_TARGET_ROLE") ? atoi(getenv("GNNMP_SM_NO_TARGET_ROLE")) : 0; if (no_tgt) p.tgt_flag = nullptr; }      // experiments
    p.cand_cap = b->max_edges + kSmK * b->max_path;
    if (p.cand_cap < 1) p.cand_cap = 1;
    p.samp_cap = b->max_samples > 0 ? b->max_samples : 0; p.path_cap = b->max_path > 0 ? b->max_path : 0;
    p.n_etiles = c.ecap / 32; p.n_ptiles = c.pcap / 32;
    p.one_free = b->total_free; p.one_coll = b->total_collided; p.init_from_path = 0; p.out = nullptr;
}

}  // namespace

extern "C" int64_t gnnmp_smoother_grad_floats(const gnnmp_smoother* h) { return h ? h->n_raw : GNNMP_ERR_NULL; }

extern "C" int gnnmp_smoother_train_workspace_bytes(const gnnmp_smoother* h, const gnnmp_smooth_batch* shape, int loop, size_t* bytes) {
    if (!h || !shape || !bytes) return GNNMP_ERR_NULL;
    if (loop < 0) return GNNMP_ERR_ARG;
    if (!sm_train_ok(h, shape)) return GNNMP_ERR_DIMS;
    SmCarve c;
    if (!sm_carve(h, shape, c)) return GNNMP_ERR_ARG;
    SmTrainCarve t;
    sm_train_carve(h, shape, loop, c, t);
    *bytes = t.inf_bytes + t.total_floats * sizeof(float);
    return GNNMP_OK;
}

// This pair is NOT the batched pair at B = 1: it runs t_bn_fwd / t_bn_bwd and sums the BatchNorm gradients in place, the batched
// one the _seg kernels and bnpart + t_bn_seg_dgb, and the suite holds the two together within a tolerance only, so folding them
// changes result bits: pin those first.
extern "C" int gnnmp_smoother_train_forward(const gnnmp_smoother* h, const gnnmp_smooth_batch* b, int loop, float* out_path,
                                            float* bn_stats, void* ws, size_t ws_bytes, void* hip_stream) {
    if (!h || !b || !ws || !out_path) return GNNMP_ERR_NULL;
    if (loop < 0) return GNNMP_ERR_ARG;
    if (!sm_train_ok(h, b)) return GNNMP_ERR_DIMS;
    SmCarve c;
    if (!sm_carve(h, b, c)) return GNNMP_ERR_ARG;
    SmTrainCarve t;
    sm_train_carve(h, b, loop, c, t);
    if (ws_bytes < t.inf_bytes + t.total_floats * sizeof(float) || (reinterpret_cast<uintptr_t>(ws) & 255)) return GNNMP_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    float* T = reinterpret_cast<float*>(static_cast<char*>(ws) + t.inf_bytes);
    const int d = h->dims.embed_size, C = h->dims.config_size, P = b->total_path, F = b->total_free, Co = b->total_collided;
    const int Nn = t.Nn, K0 = t.K0, Ec = t.ecap;
    SmParams p;
    sm_fill_params(h, b, c, ws, p);
    if ((size_t)2 * p.cand_cap * sizeof(int) > 60000) return GNNMP_ERR_DIMS;
    const auto [nc0, bn, nc3, l00, l02, l10, l12, sn] = sm_weights(h, nullptr);
    float* states = T + t.states;
    HIP_TRY(hipMemsetAsync(T, 0, t.total_floats * sizeof(float), st));                         // edge slots past the count stay finite
    HIP_TRY(launch_sm_init(P * C, p.scale, b->path, states, st));                              // model_smoother.py:118
    for (int it = 0; it < loop; ++it) {
        float* I = T + t.it0 + t.it_stride * (size_t)it;
        float* cur = states + (size_t)it * P * C;
        p.cur = cur; p.cur_next = cur;
        HIP_TRY(hipMemsetAsync(at<char>(ws, c.ff_beg), 0xFF, c.ff_end - c.ff_beg, st));
        HIP_TRY(launch_sm_knn_edges(p, st));                                                    // :125-128
        HIP_TRY(hipMemcpyAsync(I + t.esrc, p.e_src, sizeof(int) * Ec, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(I + t.edst, p.e_dst, sizeof(int) * Ec, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(I + t.ne, p.e_count, sizeof(int), hipMemcpyDeviceToDevice, st));
        const int* ne = reinterpret_cast<const int*>(I + t.ne);
        const int* es = reinterpret_cast<const int*>(I + t.esrc);
        const int* ed = reinterpret_cast<const int*>(I + t.edst);
        HIP_TRY(t_sm_nodes_in(P, F, Co, C, p.scale, cur, b->free_pts, b->collided, I + t.Xin, st));   // :130-135
        HIP_TRY(t_linear(Nn, K0, d, I + t.Xin, nc0.w, nc0.b, I + t.X0, false, st));
        HIP_TRY(t_bn_fwd(Nn, d, I + t.X0, bn.w, bn.b, I + t.X1, I + t.stats, true, st));       // BatchNorm, batch statistics + ReLU
        HIP_TRY(t_linear(Nn, d, d, I + t.X1, nc3.w, nc3.b, I + t.X, false, st));
        HIP_TRY(t_sm_msg_in(ne, d, es, ed, I + t.X, T + t.Zin, Ec, st));                       // :36-37
        HIP_TRY(t_linear(Ec, 3 * d, d, T + t.Zin, l00.w, l00.b, I + t.Zh, true, st));
        HIP_TRY(t_linear(Ec, d, d, I + t.Zh, l02.w, l02.b, T + t.M, false, st));
        HIP_TRY(t_fill((size_t)P * d, I + t.S, 0.f, st));
        HIP_TRY(t_sm_scatter_add(ne, d, ed, T + t.M, I + t.S, P, st));                        // aggr = 'add' (:32)
        HIP_TRY(t_linear(P, d, d, I + t.S, l10.w, l10.b, I + t.L1h, true, st));
        HIP_TRY(t_linear(P, d, d, I + t.L1h, l12.w, l12.b, T + t.tmpP, false, st));
        HIP_TRY(t_add_rows((size_t)P * d, I + t.X, T + t.tmpP, I + t.Hh, st));                 // x + lin_1(out) (:34), rows < P
        HIP_TRY(t_linear(P, d, C, I + t.Hh, sn.w, sn.b, T + t.prop, false, st));
        HIP_TRY(t_sm_path_update(P, C, cur, T + t.prop, cur + (size_t)P * C, st));             // :139
        if (bn_stats) {
            HIP_TRY(hipMemcpyAsync(bn_stats + (size_t)it * 2 * d, I + t.stats, sizeof(float) * d, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(bn_stats + (size_t)it * 2 * d + d, I + t.stats + 2 * d, sizeof(float) * d, hipMemcpyDeviceToDevice, st));
        }
    }
    HIP_TRY(t_scale(P * C, p.scale, states + (size_t)loop * P * C, out_path, st));                  // :142
    return GNNMP_OK;
}

extern "C" int gnnmp_smoother_train_backward(const gnnmp_smoother* h, const gnnmp_smooth_batch* b, int loop, const float* d_out_path,
                                             float* grad, void* ws, size_t ws_bytes, void* hip_stream) {
    if (!h || !b || !ws || !grad || !d_out_path) return GNNMP_ERR_NULL;
    if (loop < 0) return GNNMP_ERR_ARG;
    if (!sm_train_ok(h, b)) return GNNMP_ERR_DIMS;
    SmCarve c;
    if (!sm_carve(h, b, c)) return GNNMP_ERR_ARG;
    SmTrainCarve t;
    sm_train_carve(h, b, loop, c, t);
    if (ws_bytes < t.inf_bytes + t.total_floats * sizeof(float) || (reinterpret_cast<uintptr_t>(ws) & 255)) return GNNMP_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    float* T = reinterpret_cast<float*>(static_cast<char*>(ws) + t.inf_bytes);
    const int d = h->dims.embed_size, C = h->dims.config_size, P = b->total_path;
    const int Nn = t.Nn, K0 = t.K0, Ec = t.ecap;
    HIP_TRY(hipMemsetAsync(grad, 0, (size_t)h->n_raw * sizeof(float), st));
    const auto [nc0, bn, nc3, l00, l02, l10, l12, sn] = sm_weights(h, grad);
    float* dcur = T + t.dpa;
    float* dprev = T + t.dpb;
    HIP_TRY(t_scale(P * C, h->dims.scale, d_out_path, dcur, st));
    for (int it = loop - 1; it >= 0; --it) {
        float* I = T + t.it0 + t.it_stride * (size_t)it;
        const int* ne = reinterpret_cast<const int*>(I + t.ne);
        const int* es = reinterpret_cast<const int*>(I + t.esrc);
        const int* ed = reinterpret_cast<const int*>(I + t.edst);
        HIP_TRY(t_sm_path_update_bwd(P, C, dcur, T + t.dprop, dprev, st));
        HIP_TRY(t_linear_dw(P, d, C, T + t.dprop, I + t.Hh, sn.gw, sn.gb, T + t.dwp, st));
        HIP_TRY(t_linear_dx(P, d, C, T + t.dprop, sn.w, T + t.dHh, false, st));
        HIP_TRY(t_fill((size_t)Nn * d, T + t.dX, 0.f, st));
        HIP_TRY(hipMemcpyAsync(T + t.dX, T + t.dHh, sizeof(float) * P * d, hipMemcpyDeviceToDevice, st));   // x + ...: identity branch
        HIP_TRY(t_linear_dw(P, d, d, T + t.dHh, I + t.L1h, l12.gw, l12.gb, T + t.dwp, st));
        HIP_TRY(t_linear_dx(P, d, d, T + t.dHh, l12.w, T + t.dL1h, false, st));
        HIP_TRY(t_relu_bwd((size_t)P * d, I + t.L1h, T + t.dL1h, st));
        HIP_TRY(t_linear_dw(P, d, d, T + t.dL1h, I + t.S, l10.gw, l10.gb, T + t.dwp, st));
        HIP_TRY(t_linear_dx(P, d, d, T + t.dL1h, l10.w, T + t.dS, false, st));
        HIP_TRY(t_sm_scatter_add_bwd(ne, d, ed, T + t.dS, T + t.M, Ec, st));                    // dM
        HIP_TRY(t_linear_dw(Ec, d, d, T + t.M, I + t.Zh, l02.gw, l02.gb, T + t.dwp, st));
        HIP_TRY(t_linear_dx(Ec, d, d, T + t.M, l02.w, T + t.dZh, false, st));
        HIP_TRY(t_relu_bwd((size_t)Ec * d, I + t.Zh, T + t.dZh, st));
        HIP_TRY(t_sm_msg_in(ne, d, es, ed, I + t.X, T + t.Zin, Ec, st));                        // Zin recomputed
        HIP_TRY(t_linear_dw(Ec, 3 * d, d, T + t.dZh, T + t.Zin, l00.gw, l00.gb, T + t.dwp, st));
        HIP_TRY(t_linear_dx(Ec, 3 * d, d, T + t.dZh, l00.w, T + t.dZin, false, st));
        HIP_TRY(t_sm_msg_in_bwd(ne, d, es, ed, T + t.dZin, T + t.dX, Nn, st));
        HIP_TRY(t_linear_dw(Nn, d, d, T + t.dX, I + t.X1, nc3.gw, nc3.gb, T + t.dwp, st));
        HIP_TRY(t_linear_dx(Nn, d, d, T + t.dX, nc3.w, T + t.dX1, false, st));
        HIP_TRY(t_relu_bwd((size_t)Nn * d, I + t.X1, T + t.dX1, st));
        HIP_TRY(t_bn_bwd(Nn, d, I + t.X0, T + t.dX1, bn.w, I + t.stats, T + t.dX0, bn.gw, bn.gb, st));
        HIP_TRY(t_linear_dw(Nn, K0, d, T + t.dX0, I + t.Xin, nc0.gw, nc0.gb, T + t.dwp, st));
        HIP_TRY(t_linear_dx(Nn, K0, d, T + t.dX0, nc0.w, T + t.dXin, false, st));
        HIP_TRY(t_sm_coords_bwd(P, C, T + t.dXin, dprev, st));                                  // nodes[:P] = path (:140)
        float* sw = dcur; dcur = dprev; dprev = sw;
    }
    return GNNMP_OK;
}

// ---------------------------------------------------------------------------------------------
// the same for B problems per call, each with its own loop count (eight module calls per optimizer step at
// train_smoother.py:33-61 become one).  Problems come ordered by loop count, longest first: iteration `it` runs the
// prefix of problems with loops[b] > it, the others keep their state and contribute nothing (SmSeg, train_kernels.hip).
// ---------------------------------------------------------------------------------------------
namespace {

struct SmBatchCarve {
    SmTrainCarve t;
    size_t bnpart;           // [max_loop][B][2][d] per-problem sums for dgamma / dbeta
    size_t total_floats;
};

// the per-problem carve at B problems (max_loop >= 1: sm_batch_args), then the BatchNorm partial sums
void sm_batch_carve(const gnnmp_smoother* h, const gnnmp_smooth_batch* b, int max_loop, const SmCarve& c, SmBatchCarve& q) {
    sm_train_carve(h, b, max_loop, c, q.t);
    q.bnpart = q.t.total_floats;                                  // a multiple of 64 floats, like every slot
    const size_t n = (size_t)max_loop * b->n_problems * 2 * h->dims.embed_size;
    q.t.total_floats = q.total_floats = q.bnpart + ((n + 63) & ~(size_t)63);
}

// GNNMP_OK and the largest loop count, or the error of the argument checks shared by the three entry points
int sm_batch_args(const gnnmp_smoother* h, const gnnmp_smooth_batch* b, const int32_t* loops, int* max_loop) {
    if (b->n_problems < 1) return GNNMP_ERR_ARG;
    for (int i = 0; i < b->n_problems; ++i) {
        if (loops[i] < 1) return GNNMP_ERR_ARG;
        if (i > 0 && loops[i] > loops[i - 1]) return GNNMP_ERR_ARG;          // longest first
    }
    if (h->dims.mlp_dtype != GNNMP_F32 || b->total_path < 1 || b->max_samples > 2048) return GNNMP_ERR_DIMS;
    if ((size_t)2 * (size_t)(b->max_edges + kSmK * b->max_path) * sizeof(int) > 60000) return GNNMP_ERR_DIMS;
    *max_loop = loops[0];
    return GNNMP_OK;
}

int sm_active(const gnnmp_smooth_batch* b, const int32_t* loops, int it) {
    int a = 0;
    while (a < b->n_problems && loops[a] > it) ++a;
    return a;
}

SmSeg sm_seg(const gnnmp_smooth_batch* b, const SmTrainCarve& t) {
    SmSeg g;
    g.path_ptr = b->path_ptr; g.free_ptr = b->free_ptr; g.coll_ptr = b->coll_ptr; g.edge_ptr = b->edge_ptr;
    g.B = b->n_problems; g.A = 0; g.P = b->total_path; g.Nn = t.Nn; g.Ec = t.ecap;
    return g;
}

}  // namespace

extern "C" int gnnmp_smoother_train_batch_workspace_bytes(const gnnmp_smoother* h, const gnnmp_smooth_batch* shape, const int32_t* loops_host,
                                                          size_t* bytes) {
    if (!h || !shape || !loops_host || !bytes) return GNNMP_ERR_NULL;
    int L = 0;
    const int rc = sm_batch_args(h, shape, loops_host, &L);
    if (rc != GNNMP_OK) return rc;
    SmCarve c;
    if (!sm_carve(h, shape, c)) return GNNMP_ERR_ARG;
    SmBatchCarve q;
    sm_batch_carve(h, shape, L, c, q);
    *bytes = q.t.inf_bytes + q.total_floats * sizeof(float);
    return GNNMP_OK;
}

extern "C" int gnnmp_smoother_train_batch_forward(const gnnmp_smoother* h, const gnnmp_smooth_batch* b, const int32_t* loops_host,
                                                  float* out_path, float* bn_stats, void* ws, size_t ws_bytes, void* hip_stream) {
    if (!h || !b || !loops_host || !ws || !out_path) return GNNMP_ERR_NULL;
    if (!b->path_ptr || !b->free_ptr || !b->coll_ptr || !b->edge_ptr) return GNNMP_ERR_NULL;
    int L = 0;
    const int rc = sm_batch_args(h, b, loops_host, &L);
    if (rc != GNNMP_OK) return rc;
    SmCarve c;
    if (!sm_carve(h, b, c)) return GNNMP_ERR_ARG;
    SmBatchCarve q;
    sm_batch_carve(h, b, L, c, q);
    const SmTrainCarve& t = q.t;
    if (ws_bytes < t.inf_bytes + q.total_floats * sizeof(float) || (reinterpret_cast<uintptr_t>(ws) & 255)) return GNNMP_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    float* T = reinterpret_cast<float*>(static_cast<char*>(ws) + t.inf_bytes);
    const int d = h->dims.embed_size, C = h->dims.config_size, P = b->total_path, B = b->n_problems;
    const int Nn = t.Nn, K0 = t.K0, Ec = t.ecap;
    SmParams p;
    sm_fill_params(h, b, c, ws, p);
    SmSeg g = sm_seg(b, t);
    const auto [nc0, bn, nc3, l00, l02, l10, l12, sn] = sm_weights(h, nullptr);
    float* states = T + t.states;
    // rows no kernel writes (problems past their loop count, padding slots of the edge space) must hold finite numbers:
    // the weight gradients sum 0 * activation over them
    HIP_TRY(hipMemsetAsync(T, 0, q.total_floats * sizeof(float), st));
    if (bn_stats) HIP_TRY(hipMemsetAsync(bn_stats, 0, (size_t)B * L * 2 * d * sizeof(float), st));
    HIP_TRY(launch_sm_init(P * C, p.scale, b->path, states, st));                              // model_smoother.py:118
    for (int it = 0; it < L; ++it) {
        float* I = T + t.it0 + t.it_stride * (size_t)it;
        float* cur = states + (size_t)it * P * C;
        g.A = sm_active(b, loops_host, it);
        // the graph stage of the active prefix writes this iteration's edge list straight into its kept slots
        p.B = g.A; p.cur = cur; p.cur_next = cur;
        p.e_src = reinterpret_cast<int*>(I + t.esrc); p.e_dst = reinterpret_cast<int*>(I + t.edst); p.e_count = reinterpret_cast<int*>(I + t.ne);
        HIP_TRY(hipMemsetAsync(at<char>(ws, c.ff_beg), 0xFF, c.ff_end - c.ff_beg, st));
        HIP_TRY(launch_sm_knn_edges(p, st));                                                    // :125-128
        const int *ne = p.e_count, *es = p.e_src, *ed = p.e_dst;
        HIP_TRY(t_sm_nodes_in_seg(g, C, p.scale, cur, b->free_pts, b->collided, I + t.Xin, st));   // :130-135
        HIP_TRY(t_linear(Nn, K0, d, I + t.Xin, nc0.w, nc0.b, I + t.X0, false, st));
        HIP_TRY(t_bn_seg_fwd(g, d, I + t.X0, bn.w, bn.b, I + t.X1, I + t.stats, bn_stats ? bn_stats + (size_t)it * 2 * d : nullptr,
                             (size_t)L * 2 * d, true, st));                                    // BatchNorm per problem + ReLU
        HIP_TRY(t_linear(Nn, d, d, I + t.X1, nc3.w, nc3.b, I + t.X, false, st));
        HIP_TRY(t_sm_msg_in_seg(g, ne, d, es, ed, I + t.X, T + t.Zin, st));                    // :36-37
        HIP_TRY(t_linear(Ec, 3 * d, d, T + t.Zin, l00.w, l00.b, I + t.Zh, true, st));
        HIP_TRY(t_linear(Ec, d, d, I + t.Zh, l02.w, l02.b, T + t.M, false, st));
        HIP_TRY(t_sm_scatter_add_seg(g, ne, d, ed, T + t.M, I + t.S, st));                     // aggr = 'add' (:32)
        HIP_TRY(t_linear(P, d, d, I + t.S, l10.w, l10.b, I + t.L1h, true, st));
        HIP_TRY(t_linear(P, d, d, I + t.L1h, l12.w, l12.b, T + t.tmpP, false, st));
        HIP_TRY(t_sm_add_path_seg(g, d, I + t.X, T + t.tmpP, I + t.Hh, st));                   // x + lin_1(out) (:34), path rows
        HIP_TRY(t_linear(P, d, C, I + t.Hh, sn.w, sn.b, T + t.prop, false, st));
        HIP_TRY(t_sm_path_update_seg(g, C, cur, T + t.prop, cur + (size_t)P * C, st));         // :139
    }
    HIP_TRY(t_scale(P * C, p.scale, states + (size_t)L * P * C, out_path, st));                // :142
    return GNNMP_OK;
}

extern "C" int gnnmp_smoother_train_batch_backward(const gnnmp_smoother* h, const gnnmp_smooth_batch* b, const int32_t* loops_host,
                                                   const float* d_out_path, float* grad, void* ws, size_t ws_bytes, void* hip_stream) {
    if (!h || !b || !loops_host || !ws || !grad || !d_out_path) return GNNMP_ERR_NULL;
    if (!b->path_ptr || !b->free_ptr || !b->coll_ptr || !b->edge_ptr) return GNNMP_ERR_NULL;
    int L = 0;
    const int rc = sm_batch_args(h, b, loops_host, &L);
    if (rc != GNNMP_OK) return rc;
    SmCarve c;
    if (!sm_carve(h, b, c)) return GNNMP_ERR_ARG;
    SmBatchCarve q;
    sm_batch_carve(h, b, L, c, q);
    const SmTrainCarve& t = q.t;
    if (ws_bytes < t.inf_bytes + q.total_floats * sizeof(float) || (reinterpret_cast<uintptr_t>(ws) & 255)) return GNNMP_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    float* T = reinterpret_cast<float*>(static_cast<char*>(ws) + t.inf_bytes);
    const int d = h->dims.embed_size, C = h->dims.config_size, P = b->total_path, B = b->n_problems;
    const int Nn = t.Nn, K0 = t.K0, Ec = t.ecap;
    SmSeg g = sm_seg(b, t);
    HIP_TRY(hipMemsetAsync(grad, 0, (size_t)h->n_raw * sizeof(float), st));
    const auto [nc0, bn, nc3, l00, l02, l10, l12, sn] = sm_weights(h, grad);
    float* dcur = T + t.dpa;
    float* dprev = T + t.dpb;
    HIP_TRY(t_scale(P * C, h->dims.scale, d_out_path, dcur, st));
    for (int it = L - 1; it >= 0; --it) {
        float* I = T + t.it0 + t.it_stride * (size_t)it;
        const int* ne = reinterpret_cast<const int*>(I + t.ne);
        const int* es = reinterpret_cast<const int*>(I + t.esrc);
        const int* ed = reinterpret_cast<const int*>(I + t.edst);
        g.A = sm_active(b, loops_host, it);
        // every adjoint below is zero on the rows of problems that did not run this iteration: their d_out passes through
        HIP_TRY(t_sm_path_update_bwd_seg(g, C, dcur, T + t.dprop, dprev, st));
        HIP_TRY(t_linear_dw(P, d, C, T + t.dprop, I + t.Hh, sn.gw, sn.gb, T + t.dwp, st));
        HIP_TRY(t_linear_dx(P, d, C, T + t.dprop, sn.w, T + t.dHh, false, st));
        HIP_TRY(t_sm_add_path_bwd_seg(g, d, T + t.dHh, T + t.dX, st));                          // x + ...: identity branch
        HIP_TRY(t_linear_dw(P, d, d, T + t.dHh, I + t.L1h, l12.gw, l12.gb, T + t.dwp, st));
        HIP_TRY(t_linear_dx(P, d, d, T + t.dHh, l12.w, T + t.dL1h, false, st));
        HIP_TRY(t_relu_bwd((size_t)P * d, I + t.L1h, T + t.dL1h, st));
        HIP_TRY(t_linear_dw(P, d, d, T + t.dL1h, I + t.S, l10.gw, l10.gb, T + t.dwp, st));
        HIP_TRY(t_linear_dx(P, d, d, T + t.dL1h, l10.w, T + t.dS, false, st));
        HIP_TRY(t_sm_scatter_add_bwd_seg(g, ne, d, ed, T + t.dS, T + t.M, st));                 // dM
        HIP_TRY(t_linear_dw(Ec, d, d, T + t.M, I + t.Zh, l02.gw, l02.gb, T + t.dwp, st));
        HIP_TRY(t_linear_dx(Ec, d, d, T + t.M, l02.w, T + t.dZh, false, st));
        HIP_TRY(t_relu_bwd((size_t)Ec * d, I + t.Zh, T + t.dZh, st));
        HIP_TRY(t_sm_msg_in_seg(g, ne, d, es, ed, I + t.X, T + t.Zin, st));                     // Zin recomputed
        HIP_TRY(t_linear_dw(Ec, 3 * d, d, T + t.dZh, T + t.Zin, l00.gw, l00.gb, T + t.dwp, st));
        HIP_TRY(t_linear_dx(Ec, 3 * d, d, T + t.dZh, l00.w, T + t.dZin, false, st));
        HIP_TRY(t_sm_msg_in_bwd_seg(g, ne, d, es, ed, T + t.dZin, T + t.dX, st));
        HIP_TRY(t_linear_dw(Nn, d, d, T + t.dX, I + t.X1, nc3.gw, nc3.gb, T + t.dwp, st));
        HIP_TRY(t_linear_dx(Nn, d, d, T + t.dX, nc3.w, T + t.dX1, false, st));
        HIP_TRY(t_relu_bwd((size_t)Nn * d, I + t.X1, T + t.dX1, st));
        HIP_TRY(t_bn_seg_bwd(g, d, I + t.X0, T + t.dX1, bn.w, I + t.stats, T + t.dX0, T + q.bnpart + (size_t)it * B * 2 * d, st));
        HIP_TRY(t_linear_dw(Nn, K0, d, T + t.dX0, I + t.Xin, nc0.gw, nc0.gb, T + t.dwp, st));
        HIP_TRY(t_linear_dx(Nn, K0, d, T + t.dX0, nc0.w, T + t.dXin, false, st));
        HIP_TRY(t_sm_coords_bwd_seg(g, C, T + t.dXin, dprev, st));                              // nodes[:P] = path (:140)
        float* sw = dcur; dcur = dprev; dprev = sw;
    }
    HIP_TRY(t_bn_seg_dgb(L, B, d, T + q.bnpart, bn.gw, bn.gb, st));
    return GNNMP_OK;
}

// =============================================================================================
// supervision of the explorer's training step (train_explorer.py:124-176, train_episode_kernels.hip)
// =============================================================================================
namespace {
struct EpCarve { size_t row_beg, rev, explored, key, key_col, key_slot, dead, colkill, done, total; };
bool ep_graphs_ok(const gnnmp_episode_graphs* g) {
    return g->n_problems >= 1 && g->total_nodes >= 0 && g->total_edges >= 0 && g->node_ptr && g->edge_ptr &&
           (g->total_edges == 0 || g->edge_index);
}
void ep_carve(const gnnmp_episode_graphs* g, EpCarve& c) {
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    const size_t n1 = (size_t)g->total_nodes + g->n_problems, n2 = (size_t)g->total_nodes + 2 * (size_t)g->n_problems;
    const size_t e = (size_t)(g->total_edges > 0 ? g->total_edges : 1), n = (size_t)(g->total_nodes > 0 ? g->total_nodes : 1);
    c.row_beg = take(sizeof(int) * n1);
    c.rev = take(sizeof(int) * e);
    c.explored = take(sizeof(int) * n2);
    c.key = take(sizeof(unsigned) * n2);
    c.key_col = take(sizeof(int) * n2);
    c.key_slot = take(sizeof(int) * n2);
    c.dead = take(e);
    c.colkill = take(n);
    c.done = take(n);
    c.total = o;
}
int ep_ws_check(const gnnmp_episode_graphs* g, void* ws, size_t ws_bytes, EpCarve& c) {
    ep_carve(g, c);
    if (!ws) return GNNMP_ERR_NULL;
    if (ws_bytes < c.total || (reinterpret_cast<uintptr_t>(ws) & 255)) return GNNMP_ERR_WORKSPACE;
    return GNNMP_OK;
}
}  // namespace

extern "C" int gnnmp_episode_label_maze(const gnnmp_episode_graphs* g, int32_t dim, int32_t width, const double* points,
                                        const double* maps, uint8_t* edge_free, double* edge_cost, void* hip_stream) {
    if (!g || !points || !maps || !edge_free || !edge_cost) return GNNMP_ERR_NULL;
    if (!ep_graphs_ok(g) || width < 1) return GNNMP_ERR_ARG;
    if (dim != 2 && dim != 3) return GNNMP_ERR_DIMS;
    EpLabelParams p;
    p.B = g->n_problems; p.dim = dim; p.w = width; p.total_edges = g->total_edges;
    p.points = points; p.node_ptr = g->node_ptr; p.edge_ptr = g->edge_ptr;
    p.edge_index = reinterpret_cast<const long long*>(g->edge_index); p.maps = maps;
    p.edge_free = edge_free; p.edge_cost = edge_cost;
    if (g->total_edges > 0) HIP_TRY(launch_ep_label(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_episode_workspace_bytes(const gnnmp_episode_graphs* g, size_t* bytes) {
    if (!g || !bytes) return GNNMP_ERR_NULL;
    if (!ep_graphs_ok(g)) return GNNMP_ERR_ARG;
    EpCarve c;
    ep_carve(g, c);
    *bytes = c.total;
    return GNNMP_OK;
}

extern "C" int gnnmp_episode_paths(const gnnmp_episode_graphs* g, const double* edge_cost, const int32_t* goal_index,
                                   double* dist, int32_t* prev, int32_t* n_valid, void* ws, size_t ws_bytes, void* hip_stream) {
    if (!g || !goal_index || !dist || !prev || !n_valid) return GNNMP_ERR_NULL;
    if (!ep_graphs_ok(g)) return GNNMP_ERR_ARG;
    if (g->total_edges > 0 && !edge_cost) return GNNMP_ERR_NULL;
    EpCarve c;
    if (const int s = ep_ws_check(g, ws, ws_bytes, c)) return s;
    EpPathsParams p;
    p.B = g->n_problems; p.total_edges = g->total_edges;
    p.node_ptr = g->node_ptr; p.edge_ptr = g->edge_ptr; p.goal_index = goal_index;
    p.edge_index = reinterpret_cast<const long long*>(g->edge_index); p.edge_cost = edge_cost;
    p.dist = dist; p.prev = prev; p.n_valid = n_valid;
    p.row_beg = at<int>(ws, c.row_beg); p.done = at<unsigned char>(ws, c.done);
    HIP_TRY(launch_ep_paths(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

namespace {
int ep_episode_launch(const gnnmp_episode_graphs* g, int replay, const float* scores, const uint8_t* edge_free,
                      const int32_t* goal_index, const int32_t* start_index, const int32_t* n_valid, int32_t max_steps,
                      const double* dist, const int32_t* prev, int32_t* step, int32_t* status, int32_t* frontier,
                      int32_t* frontier_len, int32_t* label, void* ws, size_t ws_bytes, void* hip_stream) {
    if (!g || !goal_index || !start_index || !n_valid || !step || !status) return GNNMP_ERR_NULL;
    if (!ep_graphs_ok(g)) return GNNMP_ERR_ARG;
    if (g->total_edges > 0 && (!scores || !edge_free)) return GNNMP_ERR_NULL;
    if (replay && (!dist || !prev || !frontier || !frontier_len || !label)) return GNNMP_ERR_NULL;
    if (!replay && max_steps < 0) return GNNMP_ERR_ARG;
    EpCarve c;
    if (const int s = ep_ws_check(g, ws, ws_bytes, c)) return s;
    EpEpisodeParams p;
    p.B = g->n_problems; p.replay = replay; p.max_steps = max_steps; p.total_edges = g->total_edges;
    p.node_ptr = g->node_ptr; p.edge_ptr = g->edge_ptr; p.goal_index = goal_index; p.start_index = start_index;
    p.n_valid = n_valid; p.edge_index = reinterpret_cast<const long long*>(g->edge_index);
    p.scores = scores; p.edge_free = edge_free; p.dist = dist; p.prev = prev;
    p.step = step; p.status = status; p.frontier = frontier; p.frontier_len = frontier_len; p.label = label;
    p.row_beg = at<int>(ws, c.row_beg); p.rev = at<int>(ws, c.rev); p.explored = at<int>(ws, c.explored);
    p.key = at<unsigned>(ws, c.key); p.key_col = at<int>(ws, c.key_col); p.key_slot = at<int>(ws, c.key_slot);
    p.dead = at<unsigned char>(ws, c.dead); p.colkill = at<unsigned char>(ws, c.colkill);
    HIP_TRY(launch_ep_episode(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}
}  // namespace

extern "C" int gnnmp_episode_explore(const gnnmp_episode_graphs* g, const float* scores, const uint8_t* edge_free,
                                     const int32_t* goal_index, const int32_t* start_index, const int32_t* n_valid,
                                     int32_t max_steps, int32_t* step, int32_t* status, void* ws, size_t ws_bytes,
                                     void* hip_stream) {
    return ep_episode_launch(g, 0, scores, edge_free, goal_index, start_index, n_valid, max_steps, nullptr, nullptr, step, status,
                             nullptr, nullptr, nullptr, ws, ws_bytes, hip_stream);
}

extern "C" int gnnmp_episode_frontier(const gnnmp_episode_graphs* g, const float* scores, const uint8_t* edge_free,
                                      const int32_t* goal_index, const int32_t* start_index, const int32_t* n_valid,
                                      const double* dist, const int32_t* prev, const int32_t* step, const int32_t* status,
                                      int32_t* frontier, int32_t* frontier_len, int32_t* label, void* ws, size_t ws_bytes,
                                      void* hip_stream) {
    return ep_episode_launch(g, 1, scores, edge_free, goal_index, start_index, n_valid, 0, dist, prev,
                             const_cast<int32_t*>(step), const_cast<int32_t*>(status), frontier, frontier_len, label, ws,
                             ws_bytes, hip_stream);
}

// =============================================================================================
// ranked frontier rows for the host-checked planner (frontier_kernels.hip)
// =============================================================================================
namespace {
struct FrCarve { size_t zero_beg, cnt, deg, long_cnt, zero_end, long_list, st_b, st_e, st_v, total; };
bool fr_carve(const gnnmp_frontier_batch* b, FrCarve& c) {
    if (b->n_graphs < 1 || b->total_nodes < 0 || b->total_edges < 0) return false;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    const size_t n = (size_t)(b->total_nodes > 0 ? b->total_nodes : 1), e = (size_t)(b->total_edges > 0 ? b->total_edges : 1);
    c.zero_beg = o;
    c.cnt = take(sizeof(int) * n);
    c.deg = take(sizeof(int) * n);
    c.long_cnt = take(sizeof(int));
    c.zero_end = o;
    c.long_list = take(sizeof(int) * n);
    c.st_b = take(sizeof(int) * e);
    c.st_e = take(sizeof(int) * e);
    c.st_v = take(sizeof(float) * e);
    c.total = o;
    return true;
}
}  // namespace

extern "C" int gnnmp_frontier_limits(int32_t* wave_row_cells, int32_t* block_tile_cells) {
    if (!wave_row_cells || !block_tile_cells) return GNNMP_ERR_NULL;
    *wave_row_cells = kFrWaveCells;
    *block_tile_cells = kFrTileCells;
    return GNNMP_OK;
}

extern "C" int gnnmp_frontier_workspace_bytes(const gnnmp_frontier_batch* b, size_t* bytes) {
    if (!b || !bytes) return GNNMP_ERR_NULL;
    FrCarve c;
    if (!fr_carve(b, c)) return GNNMP_ERR_ARG;
    *bytes = c.total;
    return GNNMP_OK;
}

extern "C" int gnnmp_frontier_rank(const gnnmp_frontier_batch* b, int32_t* row_beg, int32_t* row_len, int32_t* cols, float* vals,
                                   int32_t* status, void* ws, size_t ws_bytes, void* hip_stream) {
    if (!b || !row_beg || !row_len || !cols || !vals || !status || !ws) return GNNMP_ERR_NULL;
    FrCarve c;
    if (!fr_carve(b, c)) return GNNMP_ERR_ARG;
    if (!b->n_free) return GNNMP_ERR_NULL;
    if (b->n_graphs > 1 && (!b->node_ptr || !b->edge_ptr)) return GNNMP_ERR_NULL;      // one graph may leave them out
    if (b->total_edges > 0 && (!b->edge_index || !b->scores)) return GNNMP_ERR_NULL;
    if (ws_bytes < c.total || (reinterpret_cast<uintptr_t>(ws) & 255)) return GNNMP_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipMemsetAsync(at<char>(ws, c.zero_beg), 0, c.zero_end - c.zero_beg, st));
    FrontierParams p;
    p.G = b->n_graphs; p.total_nodes = b->total_nodes; p.total_edges = b->total_edges;
    p.edge_index = reinterpret_cast<const long long*>(b->edge_index); p.scores = b->scores;
    p.node_ptr = b->node_ptr; p.edge_ptr = b->edge_ptr; p.n_free = b->n_free;
    p.row_beg = row_beg; p.row_len = row_len; p.cols = cols; p.vals = vals; p.status = status;
    p.cnt = at<int>(ws, c.cnt); p.deg = at<int>(ws, c.deg); p.long_cnt = at<int>(ws, c.long_cnt);
    p.long_list = at<int>(ws, c.long_list);
    p.st_b = at<int>(ws, c.st_b); p.st_e = at<int>(ws, c.st_e); p.st_v = at<float>(ws, c.st_v);
    HIP_TRY(launch_frontier_rank(p, st));
    return GNNMP_OK;
}

// =============================================================================================
// the smoother's training targets (smoother.py:67-151, oracle_smooth_kernels.hip)
// =============================================================================================
extern "C" int gnnmp_oracle_smooth_limits(int32_t* max_waypoints, int32_t* max_width) {
    if (!max_waypoints || !max_width) return GNNMP_ERR_NULL;
    *max_waypoints = kOracleSmoothCap;
    *max_width = kOracleSmoothMaxWidth;
    return GNNMP_OK;
}

// both entry points: the same checks in the same order, ``dim`` the one width the entry point serves
static int oracle_smooth_run(const gnnmp_oracle_smooth_batch* b, int dim, double* out, uint8_t* out_is32, int32_t* out_len,
                             int64_t* checks, int32_t* status, void* hip_stream) {
    if (!b || !out || !out_is32 || !out_len || !checks || !status) return GNNMP_ERR_NULL;
    if (b->dim != dim || b->width < 1 || b->width > kOracleSmoothMaxWidth) return GNNMP_ERR_DIMS;
    if (b->n_paths < 0 || b->total_points < 0 || b->iters < 0 || b->random_iter < 0 || b->prune_iter < 0 ||
        b->stop < 0 || b->stop > 2 || (b->ratio != 0 && b->ratio != 1))
        return GNNMP_ERR_ARG;
    if (b->n_paths == 0) return GNNMP_OK;
    if (!b->path_ptr || !b->maps || (b->total_points > 0 && !b->paths)) return GNNMP_ERR_NULL;
    if ((long long)b->iters * b->random_iter > 0 && (!b->action || (!b->node_idx && !b->u))) return GNNMP_ERR_NULL;
    OracleSmoothParams p;
    p.B = b->n_paths; p.total_points = b->total_points; p.w = b->width; p.iters = b->iters; p.random_iter = b->random_iter;
    p.prune_iter = b->prune_iter; p.ratio = b->ratio; p.stop = b->stop; p.dim = dim;
    p.path_ptr = b->path_ptr; p.paths = b->paths; p.in_is32 = b->is32; p.maps = b->maps;
    p.action = b->action; p.node_idx = b->node_idx; p.u = b->u;
    p.out = out; p.out_is32 = out_is32; p.out_len = out_len; p.checks = reinterpret_cast<long long*>(checks); p.status = status;
    HIP_TRY(launch_oracle_smooth(p, static_cast<hipStream_t>(hip_stream)));
    return GNNMP_OK;
}

extern "C" int gnnmp_oracle_smooth(const gnnmp_oracle_smooth_batch* b, double* out, uint8_t* out_is32, int32_t* out_len,
                                   int64_t* checks, int32_t* status, void* hip_stream) {
    return oracle_smooth_run(b, 2, out, out_is32, out_len, checks, status, hip_stream);
}

// the stick robot, MazeEnv(dim=3): batch->dim == 3, rows of three
extern "C" int gnnmp_stick_oracle_smooth(const gnnmp_oracle_smooth_batch* b, double* out, uint8_t* out_is32,
                                         int32_t* out_len, int64_t* checks, int32_t* status, void* hip_stream) {
    return oracle_smooth_run(b, 3, out, out_is32, out_len, checks, status, hip_stream);
}

// =============================================================================================
// TEST HOOKS for the training operators (gnnmp.h): one launcher of kernels.hpp per call on the caller's buffers.  Nothing
// here restates a kernel or a dispatch rule -- the hooks only check arguments and forward them.
// =============================================================================================
namespace {

struct TrainOpSpec {
    int n_dims, n_bufs;
    unsigned optional;      // bit i: bufs[i] may be NULL
    bool geom;
    int d_dim;              // index of D in dims for a geometry operator (-1: none)
    unsigned flags;         // bit i: dims[i] is a 0 / 1 flag
    unsigned zero_ok;       // bit i: dims[i] may be 0 (the launcher returns early, or the dimension is an index); every other size
                            // must be >= 1 -- the launchers do not guard an empty grid (or N = 0 of BatchNorm)
};

constexpr unsigned kSegZero = 0x1eu;       // A, P, Nn, Ec of a segmented operator

const TrainOpSpec kTrainOps[GNNMP_TOP_COUNT] = {
    /* LINEAR             */ {4, 4, 1u << 2, false, -1, 1u << 3, 1u},
    /* LINEAR_DX          */ {4, 3, 0, false, -1, 1u << 3, 1u},
    /* LINEAR_DW          */ {3, 5, 1u << 3, false, -1, 0, 1u},
    /* RELU_BWD           */ {1, 2, 0, false, -1, 0, 0},
    /* FILL               */ {1, 1, 0, false, -1, 0, 1u},
    /* NODE_IN            */ {0, 1, 0, true, -1, 0, 0},
    /* EDGE_IN            */ {0, 1, 0, true, -1, 0, 0},
    /* H0                 */ {1, 2, 0, true, 0, 0, 0},
    /* H0_BWD             */ {1, 2, 0, true, 0, 0, 0},
    /* CONCAT             */ {3, 5, 0xe, false, -1, 0, 0},       // a1 .. a3: required up to `parts` (checked below)
    /* SPLIT              */ {5, 2, 0, false, -1, 1u << 4, 1u << 3},
    /* MSG_IN             */ {1, 4, 0, true, 0, 0, 0},
    /* MSG_IN_BWD         */ {1, 3, 0, true, 0, 0, 0},
    /* POL_IN             */ {1, 3, 0, true, 0, 0, 0},
    /* POL_IN_BWD         */ {1, 2, 0, true, 0, 0, 0},
    /* SEGMENT_MAX        */ {1, 3, 0, true, 0, 0, 0},
    /* SEGMENT_MAX_BWD    */ {2, 3, 0, false, -1, 0, 0},
    /* SCORES_OUT         */ {0, 2, 0, true, -1, 0, 0},
    /* SCORES_IN          */ {0, 2, 0, true, -1, 0, 0},
    /* SM_NODES_IN        */ {4, 4, 0x6, false, -1, 0, 6u},
    /* BN_FWD             */ {3, 5, 0, false, -1, 1u << 2, 0},
    /* BN_BWD             */ {2, 7, 0, false, -1, 0, 0},
    /* SM_MSG_IN          */ {2, 5, 0, false, -1, 0, 0},
    /* SM_MSG_IN_BWD      */ {2, 5, 0, false, -1, 0, 0},
    /* SM_SCATTER_ADD     */ {2, 4, 0, false, -1, 0, 0},
    /* SM_SCATTER_ADD_BWD */ {2, 4, 0, false, -1, 0, 0},
    /* ADD_ROWS           */ {1, 3, 0, false, -1, 0, 0},
    /* SM_PATH_UPDATE     */ {2, 3, 0, false, -1, 0, 0},
    /* SM_PATH_UPDATE_BWD */ {2, 3, 0, false, -1, 0, 0},
    /* SM_COORDS_BWD      */ {2, 2, 0, false, -1, 0, 0},
    /* SCALE              */ {1, 2, 0, false, -1, 0, 1u},
    // segmented operators: dims [B, A, P, Nn, Ec, D or C, ...], A / P / Nn / Ec may be 0 (every launcher guards an empty range)
    /* SM_NODES_IN_SEG    */ {6, 8, 0, false, -1, 0, kSegZero},
    /* BN_SEG_FWD         */ {8, 10, 1u << 9, false, -1, 1u << 6, kSegZero | 1u << 7},
    /* BN_SEG_BWD         */ {6, 10, 0, false, -1, 0, kSegZero},
    /* BN_SEG_DGB         */ {3, 3, 0, false, -1, 0, 0},
    /* SM_MSG_IN_SEG      */ {6, 9, 0, false, -1, 0, kSegZero},
    /* SM_MSG_IN_BWD_SEG  */ {6, 9, 0, false, -1, 0, kSegZero},
    /* SM_SCATTER_ADD_SEG */ {6, 8, 0, false, -1, 0, kSegZero},
    /* SM_SCATTER_ADD_BWD_SEG */ {6, 8, 0, false, -1, 0, kSegZero},
    /* SM_ADD_PATH_SEG    */ {6, 7, 0, false, -1, 0, kSegZero},
    /* SM_ADD_PATH_BWD_SEG */ {6, 6, 0, false, -1, 0, kSegZero},
    /* SM_PATH_UPDATE_SEG */ {6, 7, 0, false, -1, 0, kSegZero},
    /* SM_PATH_UPDATE_BWD_SEG */ {6, 7, 0, false, -1, 0, kSegZero},
    /* SM_COORDS_BWD_SEG  */ {6, 6, 0, false, -1, 0, kSegZero},
    /* FINAL_CAT          */ {3, 3, 0, false, -1, 0, 0},         // + n_it entries of rows[] (checked below)
    /* SEED_DH            */ {3, 3, 0, false, -1, 0, 1u << 1},
    /* LINEAR_DW_ORDER    */ {4, 5, 1u << 3, false, -1, 0, 1u | 1u << 3},
};

// want: the number of dims of this call (the operator's own, except for FINAL_CAT's row table)
int train_dims_ok(const TrainOpSpec& s, const int64_t* dims, int n_dims, int want) {
    if (n_dims != want || (n_dims > 0 && !dims)) return GNNMP_ERR_ARG;
    for (int i = 0; i < n_dims; ++i) {
        const unsigned flag = i < 32 ? (s.flags >> i) & 1u : 0u, zero_ok = i < 32 ? (s.zero_ok >> i) & 1u : 0u;
        if (dims[i] < 0 || dims[i] > 0x7fffffff) return GNNMP_ERR_ARG;
        if (flag && dims[i] > 1) return GNNMP_ERR_ARG;
        if (dims[i] == 0 && !(flag | zero_ok)) return GNNMP_ERR_ARG;
    }
    return GNNMP_OK;
}

bool train_op_is_seg(int op) { return op >= GNNMP_TOP_SM_NODES_IN_SEG && op <= GNNMP_TOP_SM_COORDS_BWD_SEG && op != GNNMP_TOP_BN_SEG_DGB; }

int train_geom_ok(const gnnmp_train_geom* g) {
    if (!g) return GNNMP_ERR_NULL;
    if (g->n_graphs < 1 || g->config_size < 1 || g->n_pad < 1 || g->e_pad < 1) return GNNMP_ERR_ARG;
    if (g->n_pad % 32 || g->e_pad % 32) return GNNMP_ERR_DIMS;
    if (!g->v || !g->goal || !g->node_ptr || !g->node_ptr_pad || !g->ntile_graph || !g->goal_node || !g->row_beg || !g->deg ||
        !g->csr || !g->out_beg || !g->out_cnt || !g->out_cur || !g->out_slot)
        return GNNMP_ERR_NULL;
    return GNNMP_OK;
}

TrainGeom to_train_geom(const gnnmp_train_geom* g) {
    TrainGeom q;
    q.G = g->n_graphs; q.C = g->config_size; q.Npad = g->n_pad; q.Epad = g->e_pad;
    q.v = g->v; q.goal = g->goal; q.node_ptr = g->node_ptr; q.node_ptr_pad = g->node_ptr_pad; q.ntile_graph = g->ntile_graph;
    q.goal_node = g->goal_node; q.row_beg = g->row_beg; q.deg = g->deg; q.csr = reinterpret_cast<const int4*>(g->csr);
    q.out_beg = g->out_beg; q.out_cnt = g->out_cnt; q.out_cur = g->out_cur; q.out_slot = g->out_slot;
    return q;
}

// the explorer's own carve (CSR, padded pointers, goal node, status words), then the out lists of the training forward
struct GeomCarve { Carve c; size_t obeg, ocnt, ocur, oslot, total; };
bool geom_carve(const gnnmp_batch* b, int C, GeomCarve& g) {
    (void)C;
    if (!carve(32, GNNMP_F32, b, g.c)) return false;        // the index arrays do not depend on the embed size
    size_t o = g.c.total;
    auto take = [&](size_t bytes) { const size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    g.obeg = take(sizeof(int) * (size_t)g.c.Npad); g.ocnt = take(sizeof(int) * (size_t)g.c.Npad);
    g.ocur = take(sizeof(int) * (size_t)g.c.Npad); g.oslot = take(sizeof(int) * (size_t)g.c.Epad);
    g.total = o;
    return true;
}

}  // namespace

extern "C" int gnnmp_prep_lds_row_capacity(int32_t nodes_per_slice) { return prep_lds_row_capacity(nodes_per_slice); }

extern "C" int gnnmp_train_geom_workspace_bytes(const gnnmp_batch* shape, int32_t config_size, size_t* bytes) {
    if (!shape || !bytes) return GNNMP_ERR_NULL;
    if (config_size < 1) return GNNMP_ERR_ARG;
    GeomCarve g;
    if (!geom_carve(shape, config_size, g)) return GNNMP_ERR_ARG;
    *bytes = g.total;
    return GNNMP_OK;
}

extern "C" int gnnmp_train_geom_build(const gnnmp_batch* b, int32_t config_size, void* ws, size_t ws_bytes,
                                      gnnmp_train_geom* out, void* hip_stream) {
    if (!b || !ws || !out) return GNNMP_ERR_NULL;
    if (config_size < 1) return GNNMP_ERR_ARG;
    GeomCarve g;
    if (!geom_carve(b, config_size, g)) return GNNMP_ERR_ARG;
    if (!b->v || !b->goal || !b->node_ptr || !b->edge_ptr || (b->total_edges > 0 && !b->edge_index)) return GNNMP_ERR_NULL;
    if (ws_bytes < g.total || (reinterpret_cast<uintptr_t>(ws) & 255)) return GNNMP_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const Carve& c = g.c;
    // obstacles are not part of the geometry: obs_ptr may be NULL (the prep stage then takes every graph's count as 0)
    const PrepParams q = prep_params(c, b, config_size, ws, false, 0x7fffffff, at<int>(ws, c.gstat));
    HIP_TRY(launch_prep(q, c.Npad, c.Epad, at<int>(ws, c.prep_hist), st));
    HIP_TRY(t_sort_csr(c.Npad, q.csr, q.row_beg, q.deg, st));
    out->n_graphs = c.G; out->config_size = config_size; out->n_pad = c.Npad; out->e_pad = c.Epad;
    out->v = b->v; out->goal = b->goal; out->node_ptr = b->node_ptr;
    out->node_ptr_pad = q.node_ptr_pad; out->ntile_graph = q.ntile_graph; out->goal_node = q.goal_node;
    out->row_beg = q.row_beg; out->deg = q.deg; out->csr = at<int32_t>(ws, c.csr);
    out->out_beg = at<int32_t>(ws, g.obeg); out->out_cnt = at<int32_t>(ws, g.ocnt);
    out->out_cur = at<int32_t>(ws, g.ocur); out->out_slot = at<int32_t>(ws, g.oslot);
    HIP_TRY(t_out_csr(to_train_geom(out), st));
    return GNNMP_OK;
}

extern "C" int64_t gnnmp_train_dw_scratch_floats(int64_t R, int64_t K, int64_t O) {
    if (R < 0 || K < 0 || O < 0 || R > 0x7fffffff || K > 0x7fffffff || O > 0x7fffffff) return GNNMP_ERR_ARG;
    return (int64_t)t_linear_dw_scratch_floats((int)R, (int)K, (int)O);
}

extern "C" int gnnmp_train_op_path(int op, const int64_t* dims, int n_dims) {
    if (op == GNNMP_TOP_LINEAR_DW_ORDER) op = GNNMP_TOP_LINEAR_DW;           // the same launcher
    if (op != GNNMP_TOP_LINEAR && op != GNNMP_TOP_LINEAR_DX && op != GNNMP_TOP_LINEAR_DW) return GNNMP_ERR_ARG;
    if (n_dims < 3 || !dims) return GNNMP_ERR_ARG;
    for (int i = 0; i < 3; ++i)
        if (dims[i] < 0 || dims[i] > 0x7fffffff) return GNNMP_ERR_ARG;
    const int K = (int)dims[1], O = (int)dims[2];
    return (op == GNNMP_TOP_LINEAR ? t_linear_mfma(K, O) : op == GNNMP_TOP_LINEAR_DX ? t_linear_dx_mfma(K, O) : t_linear_dw_mfma(K, O)) ? 1 : 0;
}

extern "C" int gnnmp_train_op(int op, const int64_t* dims, int n_dims, void* const* bufs, int n_bufs,
                              const gnnmp_train_geom* geom, float scalar, void* hip_stream) {
    if (op < 0 || op >= GNNMP_TOP_COUNT) return GNNMP_ERR_ARG;
    const TrainOpSpec& s = kTrainOps[op];
    int want = s.n_dims;
    if (op == GNNMP_TOP_FINAL_CAT) {                                // [D, it_stride, n_it, rows[0] .. rows[n_it - 1]]
        if (n_dims < 3 || !dims || dims[2] < 1 || dims[2] > kTrainBatchMaxLoop) return GNNMP_ERR_ARG;
        want = 3 + (int)dims[2];
    }
    int rc = train_dims_ok(s, dims, n_dims, want);
    if (rc != GNNMP_OK) return rc;
    if (n_bufs != s.n_bufs) return GNNMP_ERR_ARG;
    if (!bufs) return GNNMP_ERR_NULL;
    auto d = [&](int i) { return (int)dims[i]; };
    if (train_op_is_seg(op) && d(1) > d(0)) return GNNMP_ERR_ARG;                              // A inside [0, B]
    if (op == GNNMP_TOP_LINEAR_DW_ORDER && d(3) > 0 && d(3) < d(0)) return GNNMP_ERR_ARG;      // R_order: 0, or >= R
    TrainLoopRows lr{};
    if (op == GNNMP_TOP_FINAL_CAT) {
        lr.n_it = d(2);
        for (int i = 0; i < lr.n_it; ++i) {
            lr.rows[i] = d(3 + i);
            if (i > 0 && lr.rows[i] > lr.rows[i - 1]) return GNNMP_ERR_ARG;                    // longest loop first
        }
        for (int i = 0; i < lr.n_it; ++i)
            if (lr.rows[i] % 256) return GNNMP_ERR_DIMS;
        if ((d(0) != 32 && d(0) != 64) || d(1) % 4) return GNNMP_ERR_DIMS;
    }
    if (op == GNNMP_TOP_SEED_DH) {
        if (d(1) > d(0)) return GNNMP_ERR_ARG;
        if (d(0) % 256 || d(1) % 256 || (d(2) != 32 && d(2) != 64)) return GNNMP_ERR_DIMS;
    }
    unsigned optional = s.optional;
    if (op == GNNMP_TOP_CONCAT) {
        if (d(2) < 1 || d(2) > 4) return GNNMP_ERR_ARG;
        optional = (0xfu << d(2)) & 0xfu;                       // parts beyond `parts` are not read
    }
    if (op == GNNMP_TOP_SPLIT && (d(2) < 1 || d(2) > 4 || d(3) >= d(2))) return GNNMP_ERR_ARG;
    if (op == GNNMP_TOP_SM_NODES_IN) optional = (d(1) == 0 ? 2u : 0u) | (d(2) == 0 ? 4u : 0u);      // no rows: never read
    for (int i = 0; i < n_bufs; ++i)
        if (!bufs[i] && !((optional >> i) & 1)) return GNNMP_ERR_NULL;
    if (op == GNNMP_TOP_FINAL_CAT || op == GNNMP_TOP_SEED_DH)      // rows travel as float4
        for (int i = 0; i < n_bufs; ++i)
            if (reinterpret_cast<uintptr_t>(bufs[i]) & 15) return GNNMP_ERR_DIMS;
    TrainGeom q{};
    if (s.geom) {
        rc = train_geom_ok(geom);
        if (rc != GNNMP_OK) return rc;
        if (s.d_dim >= 0 && d(s.d_dim) != 32 && d(s.d_dim) != 64) return GNNMP_ERR_DIMS;
        q = to_train_geom(geom);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    auto F = [&](int i) { return static_cast<float*>(bufs[i]); };
    auto I = [&](int i) { return static_cast<int*>(bufs[i]); };
    SmSeg g{};
    if (train_op_is_seg(op)) {
        g.path_ptr = I(0); g.free_ptr = I(1); g.coll_ptr = I(2); g.edge_ptr = I(3);
        g.B = d(0); g.A = d(1); g.P = d(2); g.Nn = d(3); g.Ec = d(4);
    }
    switch (op) {
        case GNNMP_TOP_LINEAR: HIP_TRY(t_linear(d(0), d(1), d(2), F(0), F(1), F(2), F(3), d(3) != 0, st)); break;
        case GNNMP_TOP_LINEAR_DX: HIP_TRY(t_linear_dx(d(0), d(1), d(2), F(0), F(1), F(2), d(3) != 0, st)); break;
        case GNNMP_TOP_LINEAR_DW: HIP_TRY(t_linear_dw(d(0), d(1), d(2), F(0), F(1), F(2), F(3), F(4), st)); break;
        case GNNMP_TOP_RELU_BWD: HIP_TRY(t_relu_bwd((size_t)d(0), F(0), F(1), st)); break;
        case GNNMP_TOP_FILL: HIP_TRY(t_fill((size_t)d(0), F(0), scalar, st)); break;
        case GNNMP_TOP_NODE_IN: HIP_TRY(t_node_in(q, F(0), st)); break;
        case GNNMP_TOP_EDGE_IN: HIP_TRY(t_edge_in(q, F(0), st)); break;
        case GNNMP_TOP_H0: HIP_TRY(t_h0(q, d(0), F(0), F(1), st)); break;
        case GNNMP_TOP_H0_BWD: HIP_TRY(t_h0_bwd(q, d(0), F(0), F(1), st)); break;
        case GNNMP_TOP_CONCAT: HIP_TRY(t_concat(d(0), d(1), d(2), F(0), F(1), F(2), F(3), F(4), st)); break;
        case GNNMP_TOP_SPLIT: HIP_TRY(t_split(d(0), d(1), d(2), d(3), F(0), F(1), d(4) != 0, st)); break;
        case GNNMP_TOP_MSG_IN: HIP_TRY(t_msg_in(q, d(0), F(0), F(1), F(2), F(3), st)); break;
        case GNNMP_TOP_MSG_IN_BWD: HIP_TRY(t_msg_in_bwd(q, d(0), F(0), F(1), F(2), st)); break;
        case GNNMP_TOP_POL_IN: HIP_TRY(t_pol_in(q, d(0), F(0), F(1), F(2), st)); break;
        case GNNMP_TOP_POL_IN_BWD: HIP_TRY(t_pol_in_bwd(q, d(0), F(0), F(1), st)); break;
        case GNNMP_TOP_SEGMENT_MAX: HIP_TRY(t_segment_max(q, d(0), F(0), F(1), I(2), st)); break;
        case GNNMP_TOP_SEGMENT_MAX_BWD: HIP_TRY(t_segment_max_bwd(d(0), d(1), F(0), I(1), F(2), st)); break;
        case GNNMP_TOP_SCORES_OUT: HIP_TRY(t_scores_out(q, F(0), F(1), st)); break;
        case GNNMP_TOP_SCORES_IN: HIP_TRY(t_scores_in(q, F(0), F(1), st)); break;
        case GNNMP_TOP_SM_NODES_IN: HIP_TRY(t_sm_nodes_in(d(0), d(1), d(2), d(3), scalar, F(0), F(1), F(2), F(3), st)); break;
        case GNNMP_TOP_BN_FWD: HIP_TRY(t_bn_fwd(d(0), d(1), F(0), F(1), F(2), F(3), F(4), d(2) != 0, st)); break;
        case GNNMP_TOP_BN_BWD: HIP_TRY(t_bn_bwd(d(0), d(1), F(0), F(1), F(2), F(3), F(4), F(5), F(6), st)); break;
        case GNNMP_TOP_SM_MSG_IN: HIP_TRY(t_sm_msg_in(I(0), d(0), I(1), I(2), F(3), F(4), d(1), st)); break;
        case GNNMP_TOP_SM_MSG_IN_BWD: HIP_TRY(t_sm_msg_in_bwd(I(0), d(0), I(1), I(2), F(3), F(4), d(1), st)); break;
        case GNNMP_TOP_SM_SCATTER_ADD: HIP_TRY(t_sm_scatter_add(I(0), d(0), I(1), F(2), F(3), d(1), st)); break;
        case GNNMP_TOP_SM_SCATTER_ADD_BWD: HIP_TRY(t_sm_scatter_add_bwd(I(0), d(0), I(1), F(2), F(3), d(1), st)); break;
        case GNNMP_TOP_ADD_ROWS: HIP_TRY(t_add_rows((size_t)d(0), F(0), F(1), F(2), st)); break;
        case GNNMP_TOP_SM_PATH_UPDATE: HIP_TRY(t_sm_path_update(d(0), d(1), F(0), F(1), F(2), st)); break;
        case GNNMP_TOP_SM_PATH_UPDATE_BWD: HIP_TRY(t_sm_path_update_bwd(d(0), d(1), F(0), F(1), F(2), st)); break;
        case GNNMP_TOP_SM_COORDS_BWD: HIP_TRY(t_sm_coords_bwd(d(0), d(1), F(0), F(1), st)); break;
        case GNNMP_TOP_SCALE: HIP_TRY(t_scale(d(0), scalar, F(0), F(1), st)); break;
        case GNNMP_TOP_SM_NODES_IN_SEG: HIP_TRY(t_sm_nodes_in_seg(g, d(5), scalar, F(4), F(5), F(6), F(7), st)); break;
        case GNNMP_TOP_BN_SEG_FWD:
            HIP_TRY(t_bn_seg_fwd(g, d(5), F(4), F(5), F(6), F(7), F(8), F(9), (size_t)d(7), d(6) != 0, st));
            break;
        case GNNMP_TOP_BN_SEG_BWD: HIP_TRY(t_bn_seg_bwd(g, d(5), F(4), F(5), F(6), F(7), F(8), F(9), st)); break;
        case GNNMP_TOP_BN_SEG_DGB: HIP_TRY(t_bn_seg_dgb(d(0), d(1), d(2), F(0), F(1), F(2), st)); break;
        case GNNMP_TOP_SM_MSG_IN_SEG: HIP_TRY(t_sm_msg_in_seg(g, I(4), d(5), I(5), I(6), F(7), F(8), st)); break;
        case GNNMP_TOP_SM_MSG_IN_BWD_SEG: HIP_TRY(t_sm_msg_in_bwd_seg(g, I(4), d(5), I(5), I(6), F(7), F(8), st)); break;
        case GNNMP_TOP_SM_SCATTER_ADD_SEG: HIP_TRY(t_sm_scatter_add_seg(g, I(4), d(5), I(5), F(6), F(7), st)); break;
        case GNNMP_TOP_SM_SCATTER_ADD_BWD_SEG: HIP_TRY(t_sm_scatter_add_bwd_seg(g, I(4), d(5), I(5), F(6), F(7), st)); break;
        case GNNMP_TOP_SM_ADD_PATH_SEG: HIP_TRY(t_sm_add_path_seg(g, d(5), F(4), F(5), F(6), st)); break;
        case GNNMP_TOP_SM_ADD_PATH_BWD_SEG: HIP_TRY(t_sm_add_path_bwd_seg(g, d(5), F(4), F(5), st)); break;
        case GNNMP_TOP_SM_PATH_UPDATE_SEG: HIP_TRY(t_sm_path_update_seg(g, d(5), F(4), F(5), F(6), st)); break;
        case GNNMP_TOP_SM_PATH_UPDATE_BWD_SEG: HIP_TRY(t_sm_path_update_bwd_seg(g, d(5), F(4), F(5), F(6), st)); break;
        case GNNMP_TOP_SM_COORDS_BWD_SEG: HIP_TRY(t_sm_coords_bwd_seg(g, d(5), F(4), F(5), st)); break;
        case GNNMP_TOP_FINAL_CAT: HIP_TRY(t_final_cat(lr, d(0), F(0), F(1), (size_t)d(1), F(2), st)); break;
        case GNNMP_TOP_SEED_DH: HIP_TRY(t_seed_dh(d(0), d(1), d(2), F(0), F(1), F(2), st)); break;
        case GNNMP_TOP_LINEAR_DW_ORDER: HIP_TRY(t_linear_dw(d(0), d(1), d(2), F(0), F(1), F(2), F(3), F(4), st, d(3))); break;
        default: return GNNMP_ERR_ARG;
    }
    return GNNMP_OK;
}
