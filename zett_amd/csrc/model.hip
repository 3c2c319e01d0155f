// model.hip — the handle's life and everything about it that is not a forward: the ONE declaration of the model's weights, their
// upload and zett_finalize (conversion to the arithmetic type, fused and LayerNorm-folded operands), the options and the getters.
// Launches only conversions and the one-off fold kernels (rowops_launch.hip.h): no GEMM is reached from here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "forward_handle.hip.h"
#include "rowops_launch.hip.h"

using namespace zett;

namespace {

// The ONE declaration of the model's weights (names and shapes: zett_amd/dims.py weight_shapes, minus the word-embedding table,
// which nothing reads): what zett_load_weight accepts, what zett_finalize requires, converts and binds.  m.layers is sized here.
std::vector<WeightDecl> declare_weights(const zett_config& c, Model& m) {
    const int64_t H = c.hidden, I = c.intermediate, E = c.n_embd, EIN = c.n_in_embd;
    std::vector<WeightDecl> d;
    auto vec = [&](const std::string& n, std::vector<int64_t> shape, const float*& slot) { d.push_back({n, std::move(shape), nullptr, &slot}); };
    auto linear = [&](const std::string& p, int64_t n, int64_t k, Linear& l) { d.push_back({p + "weight", {n, k}, &l.w, nullptr}); vec(p + "bias", {n}, l.b); };
    auto norm = [&](const std::string& p, Affine& a) { vec(p + "weight", {H}, a.w); vec(p + "bias", {H}, a.b); };
    auto scaler = [&](const std::string& p, int64_t n, Affine& a) { vec(p + "w", {1, n}, a.w); vec(p + "b", {1, n}, a.b); };
    auto block = [&](const std::string& p, Projector& b) { linear(p + "dense1.", I, H, b.dense1); linear(p + "dense2.", H, I, b.dense2); norm(p + "ln.", b.ln); };
    if (c.embed_lang) vec("lang_embeddings.weight", {c.n_langs, H}, m.lang);
    vec("model.embeddings.token_type_embeddings.weight", {1, H}, m.token_type);
    norm("model.embeddings.LayerNorm.", m.emb_ln);
    vec("model.embeddings.position_embeddings.weight", {c.max_positions, H}, m.position);
    m.layers.resize(c.layers);
    for (int l = 0; l < c.layers; ++l) {
        const std::string p = "model.encoder.layer." + std::to_string(l) + ".";
        Layer& L = m.layers[l];
        linear(p + "attention.self.query.", H, H, L.q); linear(p + "attention.self.key.", H, H, L.k); linear(p + "attention.self.value.", H, H, L.v);
        linear(p + "attention.output.dense.", H, H, L.attn_out); norm(p + "attention.output.LayerNorm.", L.attn_ln);
        linear(p + "intermediate.dense.", I, H, L.up);
        linear(p + "output.dense.", H, I, L.down); norm(p + "output.LayerNorm.", L.out_ln);
    }
    vec("fallback_embeddings.weight", {c.n_extra, EIN}, m.fallback);
    linear("input_projection.0.", H, EIN, m.in_proj); block("input_projection.1.", m.in_block);
    block("output_projection.0.", m.head_in.block); linear("output_projection.1.", c.single_head ? EIN : E, H, m.head_in.out);
    if (c.separate_out && !c.single_head) { block("output_projection_out.0.", m.head_out.block); linear("output_projection_out.1.", E, H, m.head_out.out); }
    if (c.rescale) {
        scaler("in_scaler.", EIN, m.in_scaler); scaler("scaler.", E, m.scaler);
        if (c.separate_out) scaler("out_scaler.", E, m.out_scaler);
    }
    if (c.predict_bias) { vec("bias_projection.weight", {1, H}, m.bias.w); vec("bias_projection.bias", {1}, m.bias.b); }
    std::sort(d.begin(), d.end(), [](const WeightDecl& a, const WeightDecl& b) { return a.name < b.name; });
    return d;
}

int validate_config(const zett_config& c, int precision) {
    if (c.n_embd <= 0 || c.hidden <= 0 || c.intermediate <= 0 || c.heads <= 0 || c.layers <= 0)
        return fail(ZETT_E_INVALID, "non-positive dimension in zett_config");
    if (c.n_in_embd != (c.separate_out ? 2 * c.n_embd : c.n_embd))
        return fail(ZETT_E_INVALID, "n_in_embd must be 2*n_embd iff separate_out");
    if (c.hidden % c.heads) return fail(ZETT_E_INVALID, "hidden %d not divisible by heads %d", c.hidden, c.heads);
    const int d = c.hidden / c.heads;
    if (d < 8 || d > 512 || (d & (d - 1))) return fail(ZETT_E_INVALID, "head_dim %d unsupported (need a power of two in [8,512])", d);
    const int kq = precision == ZETT_PREC_F32 ? 32 : 64;
    for (int k : {c.n_in_embd, c.hidden, c.intermediate})
        if (k % kq) return fail(ZETT_E_INVALID, "contraction width %d is not a multiple of %d", k, kq);
    if (c.n_embd % 4) return fail(ZETT_E_INVALID, "n_embd must be a multiple of 4");
    if (c.n_extra < 1) return fail(ZETT_E_INVALID, "n_extra must be >= 1 (reference allocates max(hn_n_extra_tokens,1))");
    if (c.pad_token_id < 0) return fail(ZETT_E_INVALID, "pad_token_id is required");
    if (c.embed_lang && c.n_langs <= 0) return fail(ZETT_E_INVALID, "hn_embed_lang_id needs n_langs");
    return 0;
}

// ---- the options: one row each -----------------------------------------------------------------------------------------------------
// How a value is accepted: any (stored as value != 0), lo <= value <= hi, value >= lo, or one of gemm_variant's tiles.
enum Accept { BOOLEAN, RANGE, AT_LEAST, GEMM_VARIANT };
struct OptionRow { const char* name; size_t at, size; Accept accept; int64_t lo, hi; const char* message; };
#define OPT(field) offsetof(Options, field), sizeof(Options::field)
const OptionRow OPTIONS[] = {
    {"max_chunk_tokens", OPT(max_chunk_tokens), AT_LEAST, 1024, 0, "max_chunk_tokens must be >= 1024"},
    {"time_gemm", OPT(time_gemm), BOOLEAN, 0, 0, nullptr},
    {"cls_only_last_layer", OPT(cls_only_last), BOOLEAN, 0, 0, nullptr},
    {"pair_dedupe", OPT(pair_dedupe), BOOLEAN, 0, 0, nullptr},
    {"residual_lo", OPT(residual_lo), RANGE, 0, 2, "residual_lo must be 0 (fp32 residual stream), 1 (16-bit stream in f16 mode) or 2 (in bf16 mode too)"},
    {"concurrent_lanes", OPT(concurrent_lanes), RANGE, 0, 2, "concurrent_lanes must be 0 (never), 1 (auto) or 2 (whenever a call is one chunk of >= 512 rows)"},
    {"attention_fast", OPT(attention_fast), BOOLEAN, 0, 0, nullptr},
    {"ln_fold", OPT(ln_fold), RANGE, 0, 2, "ln_fold must be 0 (off), 1 (encoder and output heads) or 2 (encoder only: A/B)"},
    {"gemm_tail_split", OPT(gemm.gemm_tail_split), RANGE, 0, 3, "gemm_tail_split must be 0 (never), 1 (auto), 2 (cut every gemm4d launch in the middle) or 3 (128x256 tiles only)"},
    {"attention_pack", OPT(attention_pack), BOOLEAN, 0, 0, nullptr},
    {"ln_rows8", OPT(ln_rows8), BOOLEAN, 0, 0, nullptr},
    {"table_lo", OPT(table_lo), BOOLEAN, 0, 0, nullptr},
    {"gemm_group", OPT(gemm.gemm_group), RANGE, 0, 64, "gemm_group must be 0 (default: 4) .. 64"},
    {"gemm_tile_order", OPT(gemm.gemm_tile_order), RANGE, 0, 1, "gemm_tile_order must be 0 or 1"},
    {"gemm4d_min_k", OPT(gemm.gemm4d_min_k), AT_LEAST, 64, 0, "gemm4d_min_k must be >= 64"},
    {"range_accumulate", OPT(range_accumulate), BOOLEAN, 0, 0, nullptr},
    {"single_rows", OPT(single_rows), RANGE, 0, 2, "single_rows must be 0 (off), 1 (auto) or 2 (whenever a call is one chunk on one lane)"},
    {"id_qkv", OPT(id_qkv), RANGE, 0, 2, "id_qkv must be 0 (off), 1 (when possible and hidden >= 4096) or 2 (whenever possible)"},
    {"gemm_variant", OPT(gemm.gemm_variant), GEMM_VARIANT, 0, 0,
     "gemm_variant must be 0 (auto), 1 (128x128), 2 (256x256 register-staged), 3 (384x256), 7 (256x256 four-wave direct-to-LDS) or 8 (7 with the generic epilogue drain)"},
};
#undef OPT

bool accepted(const OptionRow& r, int64_t v) {
    switch (r.accept) {
        case RANGE: return v >= r.lo && v <= r.hi;
        case AT_LEAST: return v >= r.lo;
        case GEMM_VARIANT: return v == 0 || v == 1 || v == 2 || v == 3 || v == 7 || v == 8;
        default: return true;
    }
}

}  // namespace

// ---------------------------------------------------------------------------------
extern "C" {

const char* zett_last_error(void) { return g_err.c_str(); }
int zett_abi_version(void) { return ZETT_ABI_VERSION; }

int zett_create(const zett_config* cfg, int device, int precision, zett_hypernet** out) {
    if (!cfg || !out) return fail(ZETT_E_INVALID, "null argument");
    if (precision != ZETT_PREC_BF16 && precision != ZETT_PREC_F32 && precision != ZETT_PREC_F16) return fail(ZETT_E_INVALID, "unknown precision %d", precision);
    if (int rc = validate_config(*cfg, precision)) return rc;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(ZETT_E_INVALID, "device %d out of range (%d visible)", device, ndev);
    ZETT_ON_DEVICE(device);
    auto* h = new zett_hypernet();
    h->cfg = *cfg;
    h->device = device;
    h->precision = precision;
    h->decl = declare_weights(h->cfg, h->m);
    if (h->range_word.alloc(64) != hipSuccess || h->range_host.alloc(64) != hipSuccess || hipMemset(h->range_word.p, 0, 64) != hipSuccess) {
        delete h;
        return fail(ZETT_E_HIP, "allocation of the range word failed");
    }
    *out = h;
    return 0;
}

int zett_destroy(zett_hypernet* h) {
    if (!h) return 0;
    ::zett::DeviceScope _scope(h->device);
    delete h;
    return 0;
}

int zett_load_weight(zett_hypernet* h, const char* name, const void* data, int dtype, const int64_t* shape, int ndim) {
    if (!h || !name || !data || !shape || ndim < 1) return fail(ZETT_E_INVALID, "null argument");
    if (h->finalized) return fail(ZETT_E_STATE, "weights are frozen after zett_finalize");
    const std::string n(name);
    auto it = std::lower_bound(h->decl.begin(), h->decl.end(), n, [](const WeightDecl& d, const std::string& key) { return d.name < key; });
    if (it == h->decl.end() || it->name != n) return 0;   // e.g. model.embeddings.word_embeddings.weight: never read
    std::vector<int64_t> got(shape, shape + ndim);
    if (got != it->shape) {
        std::string a, b;
        for (auto v : got) a += std::to_string(v) + ",";
        for (auto v : it->shape) b += std::to_string(v) + ",";
        return fail(ZETT_E_INVALID, "%s: shape [%s] does not match the config's [%s]", name, a.c_str(), b.c_str());
    }
    ZETT_ON_DEVICE(h->device);
    size_t numel = 1;
    for (auto v : got) numel *= (size_t)v;
    Tensor& t = h->w[n];
    t.shape = got;
    t.numel = numel;
    HIP_TRY(t.f32.alloc(numel * 4));          // (an earlier upload of the same name is released first)
    if (dtype == ZETT_F32) {
        HIP_TRY(hipMemcpy(t.f32.p, data, numel * 4, hipMemcpyDefault));
    } else if (dtype == ZETT_F16 || dtype == ZETT_BF16) {
        DevMem<void> stage;
        HIP_TRY(stage.alloc(numel * 2));
        hipError_t e = hipMemcpy(stage.p, data, numel * 2, hipMemcpyDefault);
        if (e == hipSuccess) {
            const int blocks = (int)std::min<size_t>((numel + 255) / 256, 65535);
            if (dtype == ZETT_F16) hipLaunchKernelGGL(convert_to_f32_kernel<1>, dim3(blocks), dim3(256), 0, 0, stage.p, t.f32.p, numel);
            else hipLaunchKernelGGL(convert_to_f32_kernel<2>, dim3(blocks), dim3(256), 0, 0, stage.p, t.f32.p, numel);
            e = hipDeviceSynchronize();
        }
        if (e != hipSuccess) return fail(ZETT_E_HIP, "upload of %s failed: %s", name, hipGetErrorString(e));
    } else {
        return fail(ZETT_E_INVALID, "unknown dtype %d", dtype);
    }
    return 0;
}

int zett_finalize(zett_hypernet* h) {
    if (!h) return fail(ZETT_E_INVALID, "null handle");
    if (h->finalized) return 0;
    ZETT_ON_DEVICE(h->device);
    std::vector<Tensor*> ts;          // the uploaded tensor of every declared weight, in the declaration's order
    for (const WeightDecl& d : h->decl) {
        auto it = h->w.find(d.name);
        if (it == h->w.end()) return fail(ZETT_E_STATE, "missing weight: %s", d.name.c_str());
        ts.push_back(&it->second);
    }
    const zett_config& c = h->cfg;
    Model& m = h->m;
    const size_t es = elt_size(h->precision);
    const bool lo = h->precision != ZETT_PREC_F32;
    // GEMM operands in the arithmetic type (the fp32 mode reads the upload itself)
    for (size_t i = 0; lo && i < ts.size(); ++i) {
        Tensor& t = *ts[i];
        if (!h->decl[i].operand) continue;
        HIP_TRY(t.lo.alloc(t.numel * 2));
        const int blocks = (int)std::min<size_t>((t.numel / 4 + 255) / 256 + 1, 65535);
        with_precision(h->precision, [&](auto a) {
            using T = typename decltype(a)::type;
            if constexpr (sizeof(T) == 2)       // (no fp32 instantiation of the kernel exists)
                hipLaunchKernelGGL(convert_f32_to_lo_kernel<T>, dim3(blocks), dim3(256), 0, 0, t.f32.p, (T*)t.lo.p, t.numel, h->range_word.p);
        });
    }
    HIP_TRY(hipDeviceSynchronize());
    // bind the model: a GEMM operand's copy in the arithmetic type, the fp32 tensor of everything else — the tensors as they are
    // NOW, whatever order they were uploaded in and however often
    for (size_t i = 0; i < ts.size(); ++i)
        if (h->decl[i].operand) *h->decl[i].operand = lo ? ts[i]->lo.p : (void*)ts[i]->f32.p;
        else *h->decl[i].vec = ts[i]->f32.p;
    auto original = [&](const Linear& l) -> const float* {      // the fp32 original of an operand (until it is freed below)
        for (size_t i = 0; i < ts.size(); ++i)
            if (h->decl[i].operand == &l.w) return ts[i]->f32.p;
        return nullptr;
    };
    // fused QKV operand per layer: rows [q | k | v]
    const size_t H = c.hidden;
    for (Layer& L : m.layers) {
        void* wq = nullptr; float* bq = nullptr;
        HIP_TRY(h->keep(wq, 3 * H * H * es));
        HIP_TRY(h->keep(bq, 3 * H * 4));
        int k = 0;
        for (const Linear* part : {&L.q, &L.k, &L.v}) {
            HIP_TRY(hipMemcpy((char*)wq + (size_t)k * H * H * es, part->w, H * H * es, hipMemcpyDeviceToDevice));
            HIP_TRY(hipMemcpy(bq + (size_t)k * H, part->b, H * 4, hipMemcpyDeviceToDevice));
            ++k;
        }
        L.qkv = Linear{wq, bq};
    }
    // LayerNorm fold operands (rowops.hip.h fold_weight_kernel); needs the fp32 originals, which are freed below
    if (lo && c.hidden % 128 == 0) {
        auto fold = [&](const float* w32, size_t N, size_t K, const Affine& ln, const float* bias, Folded& f) -> int {
            HIP_TRY(h->keep(f.w, N * K * es));
            HIP_TRY(h->keep(f.c, N * 4));
            HIP_TRY(h->keep(f.b, N * 4));
            with_precision(h->precision, [&](auto a) {
                using T = typename decltype(a)::type;
                if constexpr (sizeof(T) == 2)
                    launch_fold_weight<T>(0, w32, (int)N, (int)K, ln.w, ln.b, bias, (T*)f.w, f.c, f.b, h->range_word.p);
            });
            return 0;
        };
        DevMem<float> tmp_mem;                      // fp32 [3H, H] fused QKV of one layer
        HIP_TRY(tmp_mem.alloc(3 * H * H * 4));
        float* const tmp = tmp_mem.p;
        for (int l = 0; l < c.layers; ++l) {
            Layer& L = m.layers[l];
            if (int rc = fold(original(L.up), c.intermediate, H, L.attn_ln, L.up.b, L.fold_up)) return rc;
            // lever 6 is possible for this configuration (what the options add: forward_mode's table_lo)
            const bool id_qkv = l == 0 && c.layers >= 2 && !c.embed_lang && H * sizeof(float) <= 64 * 1024;
            if (l == 0 && !id_qkv) continue;
            int k = 0;
            for (const Linear* part : {&L.q, &L.k, &L.v}) {
                HIP_TRY(hipMemcpy(tmp + (size_t)k * H * H, original(*part), H * H * 4, hipMemcpyDeviceToDevice));
                ++k;
            }
            if (l > 0) {
                if (int rc = fold(tmp, 3 * H, H, m.layers[l - 1].out_ln, L.qkv.b, L.fold_qkv)) return rc;
                continue;
            }
            // gamma_t (.) gamma and beta_t (.) gamma (fp32 products, made on the host), no bias: the fold of layer 0's qkv onto raw table rows
            std::vector<float> gt(H), bt(H), ge(H), g2(H), b2(H);
            HIP_TRY(hipMemcpy(gt.data(), m.in_block.ln.w, H * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(bt.data(), m.in_block.ln.b, H * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(ge.data(), m.emb_ln.w, H * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < H; ++i) { g2[i] = gt[i] * ge[i]; b2[i] = bt[i] * ge[i]; }
            DevMem<float> aux_mem;                  // [H] gamma'', [H] beta'', [3H] zero bias
            HIP_TRY(aux_mem.alloc(5 * H * 4));
            float* const aux = aux_mem.p;
            HIP_TRY(hipMemset(aux, 0, 5 * H * 4));
            HIP_TRY(hipMemcpy(aux, g2.data(), H * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(aux + H, b2.data(), H * 4, hipMemcpyHostToDevice));
            const Affine ln2{aux, aux + H};
            if (int rc = fold(tmp, 3 * H, H, ln2, aux + 2 * H, m.id_u)) return rc;
            HIP_TRY(h->keep(m.id_cpos, (size_t)c.max_positions * 3 * H * 4));
            HIP_TRY(h->keep(m.id_cw, 3 * H * 4));
            HIP_TRY(h->keep(m.id_bq, 3 * H * 4));
            launch_pos_qkv(0, tmp, (int)(3 * H), (int)H, m.emb_ln.w, m.emb_ln.b, L.qkv.b, m.token_type, m.position, c.max_positions, m.id_cpos, m.id_cw, m.id_bq);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipDeviceSynchronize());        // (aux is read by the kernels above: freed behind them)
        }
        // the output heads: Linear(LN_1e-6(.)) with the ProjectorBlock's LayerNorm folded in (not for the split single head,
        // whose two-destination epilogue is the generic one)
        if (!(c.single_head && c.separate_out)) {
            const size_t w0 = c.single_head ? c.n_in_embd : c.n_embd;      // (= n_embd: a single head is not split here)
            for (Head* hd : {&m.head_in, &m.head_out})
                if (hd->out.w)
                    if (int rc = fold(original(hd->out), w0, H, hd->block.ln, hd->out.b, hd->fold)) return rc;
            std::vector<float> ones(w0, 1.0f), zeros(w0, 0.0f);
            HIP_TRY(h->keep(m.head_one, w0 * 4));
            HIP_TRY(h->keep(m.head_zero, w0 * 4));
            HIP_TRY(hipMemcpy(m.head_one, ones.data(), w0 * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(m.head_zero, zeros.data(), w0 * 4, hipMemcpyHostToDevice));
        }
        HIP_TRY(hipDeviceSynchronize());            // (tmp is read by the fold kernels: freed behind them)
    }
    // range guard: a weight (or gamma-folded weight) that does not fit the operand type is an error here, not an inf later
    HIP_TRY(hipMemcpy(h->range_host.p, h->range_word.p, 4, hipMemcpyDeviceToHost));
    if (h->range_host.p[0] & ZETT_RANGE_WEIGHT)
        return fail(ZETT_E_RANGE, "a GEMM weight (or a LayerNorm-folded weight W*gamma) exceeds the half range (|w| > 65504 or not finite): "
                                  "this checkpoint needs ZETT_PREC_BF16 or ZETT_PREC_F32");
    // output Rescaler vectors laid out over the first head's columns
    if (c.rescale) {
        const size_t w0 = c.single_head ? c.n_in_embd : c.n_embd;
        float* scale = nullptr; float* shift = nullptr;
        HIP_TRY(h->keep(scale, w0 * 4));
        HIP_TRY(h->keep(shift, w0 * 4));
        HIP_TRY(hipMemcpy(scale, m.scaler.w, c.n_embd * 4, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(shift, m.scaler.b, c.n_embd * 4, hipMemcpyDeviceToDevice));
        if (c.single_head && c.separate_out) {
            HIP_TRY(hipMemcpy(scale + c.n_embd, m.out_scaler.w, c.n_embd * 4, hipMemcpyDeviceToDevice));
            HIP_TRY(hipMemcpy(shift + c.n_embd, m.out_scaler.b, c.n_embd * 4, hipMemcpyDeviceToDevice));
        }
        m.head_in.scale = scale; m.head_in.shift = shift;
        m.head_out.scale = m.out_scaler.w; m.head_out.shift = m.out_scaler.b;
    }
    // the fp32 originals of 16-bit GEMM operands are no longer needed
    for (size_t i = 0; lo && i < ts.size(); ++i)
        if (h->decl[i].operand) ts[i]->f32.release();
    h->finalized = true;
    return 0;
}

int zett_set_option(zett_hypernet* h, const char* key, int64_t value) {
    if (!h || !key) return fail(ZETT_E_INVALID, "null argument");
    for (const OptionRow& r : OPTIONS) {
        if (strcmp(r.name, key)) continue;
        if (!accepted(r, value)) return fail(ZETT_E_INVALID, "%s", r.message);
        if (r.accept == BOOLEAN) value = value != 0;
        char* field = (char*)&h->opt + r.at;
        if (r.size == sizeof(int64_t)) *(int64_t*)field = value;
        else *(int*)field = (int)value;
        return 0;
    }
    return fail(ZETT_E_INVALID, "unknown option %s", key);
}

int zett_get_stats(const zett_hypernet* h, zett_stats* out) {
    if (!h || !out) return fail(ZETT_E_INVALID, "null argument");
    *out = h->stats;
    return 0;
}

int zett_single_rows(const zett_hypernet* h, int64_t* out) {
    if (!h || !out) return fail(ZETT_E_INVALID, "null argument");
    *out = h->single_rows_last;
    return 0;
}

int zett_id_qkv(const zett_hypernet* h, int64_t* out) {
    if (!h || !out) return fail(ZETT_E_INVALID, "null argument");
    *out = h->id_qkv_last;
    return 0;
}

int zett_stream_wait_output(zett_hypernet* h, int which, void* stream) {
    if (!h) return fail(ZETT_E_INVALID, "null handle");
    if (which != ZETT_OUT_IN && which != ZETT_OUT_BIAS) return fail(ZETT_E_INVALID, "which must be ZETT_OUT_IN or ZETT_OUT_BIAS");
    if (!h->out_recorded) return fail(ZETT_E_STATE, "no forward has run on this handle");
    ZETT_ON_DEVICE(h->device);
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, h->out_ready[which], 0));
    return 0;
}

int zett_get_gemm_log(const zett_hypernet* h, zett_gemm_record* out, int64_t capacity, int64_t* count) {
    if (!h || !count || capacity < 0 || (capacity > 0 && !out)) return fail(ZETT_E_INVALID, "null argument");
    *count = (int64_t)h->gemm_log.size();
    for (int64_t i = 0; i < capacity && i < *count; ++i) out[i] = h->gemm_log[(size_t)i];
    return 0;
}

int zett_check_range(zett_hypernet* h, void* stream, int32_t* flags) {
    if (!h) return fail(ZETT_E_INVALID, "null handle");
    ZETT_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(h->range_host.p, h->range_word.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int32_t w = h->range_host.p[0];
    if (h->opt.range_accumulate && w) HIP_TRY(hipMemsetAsync(h->range_word.p, 0, 4, st));
    if (flags) *flags = w;
    if (!w) return 0;
    return fail(ZETT_E_RANGE, "the last forward left the range of its arithmetic:%s%s%s%s (precision %s)",
                (w & ZETT_RANGE_SOURCE) ? " in_scaler(source_embeddings) beyond the half range;" : "",
                (w & ZETT_RANGE_ACTIVATION) ? " a 16-bit activation (Q/K/V, FFN intermediate or the operand copy of the residual sum) beyond the half range;" : "",
                (w & ZETT_RANGE_OUTPUT) ? " non-finite predicted embeddings;" : "",
                (w & ZETT_RANGE_DEST) ? " a finite value beyond the range of an f16 destination (stored as inf);" : "",
                h->precision == ZETT_PREC_F16 ? "f16: re-run with ZETT_PREC_BF16" : h->precision == ZETT_PREC_BF16 ? "bf16" : "f32");
}

}  // extern "C"
