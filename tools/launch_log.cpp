// Launch recorder: which kernel instance, grid, block and dynamic LDS size does libec_amd.so launch for a call?  Host only, no
// GPU and no HIP headers: this program DEFINES the HIP runtime entry points the library imports (`nm -D --undefined-only`),
// loads the library with dlopen and drives it with fake device addresses.  Linked with -rdynamic, so the definitions here
// come first in the library's symbol lookup.
//
//   c++ -O1 -std=c++17 -rdynamic -o launch_log tools/launch_log.cpp -ldl
//   launch_log LIB [--args N | --args-of SUBSTR N [INDEX] ...] < commands
//
// Commands, one per line (tests/golden/make_conv_routes_golden.py writes them):
//   conv  B H W Cin Cout ksize pool act res ldo     ec_conv_bf16 (ldo = 0) / ec_conv_bf16_ld
//   s2    B H W Cin Cout ksize act res              ec_conv_bf16_s2
//   gemm  M N K act res                             ec_gemm_bf16
//   x3    M N K act                                 ec_gemm_bf16a_x3
//   f32   M N K sam sak sbk sbn ldc flags bias gbias gidx group dmask rowscale splitk aoff boff
//                                                   ec_gemm_f32; bias .. rowscale (but group) are 0 / 1 = NULL / a fake pointer;
//                                                   aoff / boff: byte offsets of A / B from a 1 MiB-aligned base
//   pair  M K0 N N2 two res                         ec_conv1x1_pair_bf16 (two: the second product a1 . w1^T + b1; res: the residual)
//   pairpool B H W K0 N N2 y                        ec_conv1x1_pair_pool_bf16 (y = 0: y = NULL, not stored)
//   img   B H C pool ldo                            ec_conv3x3_img_pack + ec_conv3x3_img_bf16_ld (ldo = 0: dense)
//   bneck23  B H W C                                ec_bneck_pack_weights + ec_bneck_conv23_bf16
//   bneck123 B H W C                                ec_bneck3_pack_weights + ec_bneck_conv123_bf16
//   tail  B Ho Wo planes inplanes Cout              ec_basic_tail_s2_bf16
//   trunk clip50|tv50|tv18|vitb32 frames min_tiles  create + ec_*_set_conv8_min_tiles + one forward + destroy
//   tower clip|tvb|tvbasic width l1 l2 l3 l4 res frames min_tiles chunk f32|u8|depth|rgbd
//                                                   the same for an explicit ResNet architecture (CLIP tower, torchvision
//                                                   Bottleneck / BasicBlock tower; the torchvision towers have width 64) through
//                                                   ec_rn50_forward / _u8 / _depth; `P <ec_rn50_num_ops> <ec_rn50_plan_hash>`
//                                                   comes before its launches.  rgbd: ec_rn50_embed_rgbd on fp32 RGB frames,
//                                                   `frames` and `chunk` counting pairs.  A `+l1` behind the input kind
//                                                   (f32+l1, ...): ec_rn50_set_l1_rebuild(h, 1) first, `S <rc>` in front of `P`;
//                                                   `+l1off`: on, then off again
//   rebuild M K0 N N2                               ec_conv1x1_pair_rebuild_bf16
//   policy <the first 13 ec_policy_cfg fields, in order> T N mode bf16 reuse [dhf [core [pad pnull [face]]]]
//                                                   create + ec_policy_workspace_bytes + ec_policy_forward2 (goal_in > 0:
//                                                   ec_policy_forward_vec) + destroy; mode 0 = EC_POLICY_INFER, 1 = _LEARN;
//                                                   reuse 1: an EC_POLICY_INFER call builds the tables first (`B <rc>` ends
//                                                   its launches), then the recorded call is EC_POLICY_INFER_REUSE in the
//                                                   same workspace.  mode 2: the learn pass -- the EC_POLICY_LEARN forward
//                                                   (`F <rc>` ends its launches), then ec_policy_backward2 in the same
//                                                   workspace; dhf 1 (mode 2 only): with a dh_final tensor, else NULL.
//                                                   core = 10 * rnn_type + num_layers (2: a two-layer GRU, 12: a two-layer
//                                                   LSTM): ec_policy_create_rnn_layers instead of ec_policy_create.
//                                                   pad pnull: ec_policy_cfg's prev_action_dims and prev_action_null.
//                                                   face: the entry point in place of the forward -- 1 ec_policy_act / _vec,
//                                                   2 ec_policy_act_greedy / _vec_greedy, 3 ec_policy_act_ex, 4 the same with
//                                                   forcing pointers (force_p 0.25), 5 ec_policy_forward_pa, 6 ec_policy_act_pa,
//                                                   7 the same with forcing pointers; the act faces want T = 1 and mode 0 and
//                                                   pass seed 1, step 2, first_actor 3.
//                                                   `W <bytes>` is the workspace size, `D <bytes>` a device-to-device
//                                                   hipMemcpyAsync (policy commands only)
//   pooled D H ed goals ns k0 k1 k2 A E null rnn L T N mode reuse inplace act
//                                                   ec_policy_create_pooled + ec_policy_workspace_bytes + ec_policy_forward_pooled
//                                                   (+ ec_policy_backward2 with mode 2) + destroy; mode / reuse / `W` / `B` / `F` / `D`
//                                                   as for `policy`; inplace 1: h_final == h0;
//                                                   act 1 (T = 1, mode 0): ec_policy_act_pooled, sampling, instead of the forward
//   twoview C S H A1 A E null rnn L T N mode reuse inplace act
//                                                   ec_policy_create_two_view (the nine ec_two_view_cfg fields) + the rest as for
//                                                   `pooled` with ec_policy_forward_two_view, both views bf16; act 1 (T = 1,
//                                                   mode 0): ec_policy_act_two_view, sampling; act 2: with forcing pointers
//   stem  B H W Cout u8                             ec_stem_conv1 (u8 = 0) / ec_stem_conv1_u8 (the staging branch is chosen inside the
//                                                   kernel: the record is the instance and the grid)
//   stem7 B H W u8                                  ec_stem7_pool on fp32 (u8 = 0) / uint8 frames
//   dstem B H W Cout                                ec_stem_conv1_depth
//   avgpool B H W C ldo                             ec_avgpool2_bf16 (ldo = 0) / ec_avgpool2_bf16_ld
//   tonchw B HW C                                   ec_nhwc_bf16_to_nchw_f32
//   tonhwc B HW C                                   ec_nchw_f32_to_nhwc_bf16
//   mean  B HW C                                    ec_spatial_mean_bf16
// Output: `K <kernel>` per registered kernel, then per command `C <command>`, one `L <kernel>|<grid>|<block>|<lds>` per
// launch (with --args N: `|` + the first N bytes of the first kernel argument in hex, for the conv_igemm kernels; --args-of SUBSTR N:
// for the kernels whose name contains SUBSTR; --args-of SUBSTR N INDEX: of kernel argument INDEX, which has to be at least N bytes
// long; --args-of may repeat) and `R <rc>`.
#include <cxxabi.h>
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <sstream>
#include <string>
#include <vector>

struct dim3 { unsigned x, y, z; };

static std::map<const void*, std::string> g_kernels;
static struct { dim3 grid, block; size_t lds; void* stream; } g_cfg;
struct Dump { std::string of; int index, bytes; };   // kernels whose name contains `of`: the first `bytes` bytes of argument `index`
static std::vector<Dump> g_dumps;
static int g_log_copies = 0;                   // policy commands: hipMemcpyAsync is part of the recorded sequence
static uintptr_t g_next = 0x100000000000ull;   // fake device addresses; never dereferenced
static void* fake(size_t bytes) { void* p = (void*)g_next; g_next += (bytes + 0xfffff) & ~(size_t)0xfffff; return p; }

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
    int st = 0;
    char* d = abi::__cxa_demangle(device_name, nullptr, nullptr, &st);
    g_kernels[host_fn] = st == 0 ? d : device_name;
    free(d);
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
int __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, void* stream) { g_cfg = {grid, block, lds, stream}; return 0; }
int __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, void** stream) {
    *grid = g_cfg.grid; *block = g_cfg.block; *lds = g_cfg.lds; *stream = g_cfg.stream;
    return 0;
}
int hipLaunchKernel(const void* fn, dim3 g, dim3 b, void** args, size_t lds, void*) {
    auto it = g_kernels.find(fn);
    const std::string name = it == g_kernels.end() ? "?" : it->second;
    printf("L %s|%u,%u,%u|%u,%u,%u|%zu", name.c_str(), g.x, g.y, g.z, b.x, b.y, b.z, lds);
    for (const Dump& d : g_dumps) {
        if (name.find(d.of) == std::string::npos) continue;
        printf("|");
        for (int i = 0; i < d.bytes; ++i) printf("%02x", ((const unsigned char*)args[d.index])[i]);
    }
    printf("\n");
    return 0;
}
int hipGetLastError() { return 0; }
int hipGetDevice(int* d) { *d = 0; return 0; }
int hipFuncSetAttribute(const void*, int, int) { return 0; }
int hipMalloc(void** p, size_t n) { *p = fake(n); return 0; }
int hipFree(void*) { return 0; }
int hipMemcpy(void*, const void*, size_t, int) { return 0; }
int hipMemcpy2D(void*, size_t, const void*, size_t, size_t, size_t, int) { return 0; }
int hipMemcpyAsync(void*, const void*, size_t n, int, void*) {
    if (g_log_copies) printf("D %zu\n", n);
    return 0;
}
int hipMemsetAsync(void*, int, size_t, void*) { return 0; }
int hipDeviceSynchronize() { return 0; }
int hipStreamSynchronize(void*) { return 0; }
int hipStreamWaitEvent(void*, void*, unsigned) { return 0; }
int hipEventCreate(void** e) { *e = nullptr; return 0; }
int hipEventDestroy(void*) { return 0; }
int hipEventRecord(void*, void*) { return 0; }
int hipEventElapsedTime(float* ms, void*, void*) { *ms = 1.f; return 0; }
}

static void* g_lib;
template <class F>
static F sym(const char* name) {
    void* p = dlsym(g_lib, name);
    if (!p) { fprintf(stderr, "launch_log: %s not found\n", name); exit(2); }
    return (F)p;
}

// weight / bias element counts of the Bottleneck (expansion 4) and BasicBlock (expansion 1) layers, in the order ec_amd.h documents
static void resnet_counts(const int* layers, bool basic, size_t& nw, size_t& nb, size_t width = 64) {
    size_t in = width;
    for (int l = 0; l < 4; ++l) {
        const size_t p = width << l, out = basic ? p : 4 * p;
        for (int b = 0; b < layers[l]; ++b) {
            nw += basic ? p * 9 * in + p * 9 * p : p * in + p * 9 * p + out * p;
            nb += basic ? 2 * p : 2 * p + out;
            if (b == 0 && (in != out || (l > 0))) { nw += out * in; nb += out; }
            in = out;
        }
    }
}

static int run_trunk(const std::string& kind, int frames, int min_tiles) {
    typedef void* P;
    void* h = nullptr;
    int rc;
    const P w = fake(1u << 30), f = fake(1u << 28), stem = fake(1u << 20), rgb = fake(1u << 30), out = fake(1u << 30);
    if (kind == "vitb32") {
        const size_t D = 768, Kp = 32 * 32 * 3, L = 50, layers = 11;
        rc = sym<int (*)(P*, int, int, int, int, int, P, size_t, P, size_t)>("ec_vit_create")(
            &h, (int)D, (int)layers, 12, 32, 224, w, D * Kp + layers * 12 * D * D, f, D + L * D + 2 * D + layers * 13 * D);
        if (rc) return rc;
        sym<int (*)(P, int)>("ec_vit_set_conv8_min_tiles")(h, min_tiles);
        const size_t ws = sym<size_t (*)(P, int)>("ec_vit_workspace_bytes")(h, frames);
        rc = sym<int (*)(P, P, int, P, size_t, P, P)>("ec_vit_forward")(h, rgb, frames, fake(ws), ws, out, nullptr);
        sym<void (*)(P)>("ec_vit_destroy")(h);
        return rc;
    }
    const bool basic = kind == "tv18";
    const int l50[4] = {3, 4, 6, 3}, l18[4] = {2, 2, 2, 2};
    const int* layers = basic ? l18 : l50;
    size_t nw = 0, nb = 0;
    resnet_counts(layers, basic, nw, nb);
    if (kind == "clip50")   // + stem conv2 [32][9*32], conv3 [64][9*32]; biases of stem conv1..3
        rc = sym<int (*)(P*, int, const int*, int, P, P, size_t, P, size_t)>("ec_rn50_create")(
            &h, 64, layers, 224, stem, w, nw + 32 * 288 + 64 * 288, f, nb + 32 + 32 + 64);
    else
        rc = sym<int (*)(P*, const int*, int, P, P, size_t, P, size_t)>(basic ? "ec_tvresnet_basic_create" : "ec_rn50tv_create")(
            &h, layers, 224, stem, w, nw, f, nb + 64);
    if (rc) return rc;
    sym<int (*)(P, int)>("ec_rn50_set_conv8_min_tiles")(h, min_tiles);
    const size_t ws = sym<size_t (*)(P, int)>("ec_rn50_workspace_bytes")(h, frames);
    rc = sym<int (*)(P, P, int, P, size_t, P, int, P)>("ec_rn50_forward")(h, rgb, frames, fake(ws), ws, out, 0, nullptr);
    sym<void (*)(P)>("ec_rn50_destroy")(h);
    return rc;
}

// v: width, the four layer counts, resolution, frames, min_tiles, chunk
static int run_tower(const std::string& kind, const int* v, const std::string& input_) {
    typedef void* P;
    const size_t plus = input_.find('+');
    const std::string input = input_.substr(0, plus), opt = plus == std::string::npos ? "" : input_.substr(plus);
    if (!opt.empty() && opt != "+l1" && opt != "+l1off") return -100;
    const int width = v[0], *layers = v + 1, res = v[5], frames = v[6], min_tiles = v[7], chunk = v[8];
    const bool clip = kind == "clip", basic = kind == "tvbasic";
    if ((!clip && kind != "tvb" && !basic) || (!clip && width != 64) || width <= 0) return -100;
    void* h = nullptr;
    int rc;
    const P w = fake(1u << 30), f = fake(1u << 28), stem = fake(1u << 20), rgb = fake(1u << 30), out = fake(1u << 30), w9 = fake(1u << 20);
    size_t nw = 0, nb = 0;
    resnet_counts(layers, basic, nw, nb, (size_t)width);
    if (clip) {   // + stem conv2 [sc][9*sc], conv3 [width][9*sc] at the padded stem width sc; biases of stem conv1..3
        const size_t sc = ((size_t)width / 2 + 31) / 32 * 32;
        rc = sym<int (*)(P*, int, const int*, int, P, P, size_t, P, size_t)>("ec_rn50_create")(
            &h, width, layers, res, stem, w, nw + sc * 9 * sc + (size_t)width * 9 * sc, f, nb + 2 * sc + (size_t)width);
    } else {
        rc = sym<int (*)(P*, const int*, int, P, P, size_t, P, size_t)>(basic ? "ec_tvresnet_basic_create" : "ec_rn50tv_create")(
            &h, layers, res, stem, w, nw, f, nb + 64);
    }
    if (rc) return rc;
    sym<int (*)(P, int)>("ec_rn50_set_conv8_min_tiles")(h, min_tiles);
    if (!opt.empty()) printf("S %d\n", sym<int (*)(P, int)>("ec_rn50_set_l1_rebuild")(h, 1));
    if (opt == "+l1off") printf("S %d\n", sym<int (*)(P, int)>("ec_rn50_set_l1_rebuild")(h, 0));
    printf("P %d %016llx\n", sym<int (*)(P)>("ec_rn50_num_ops")(h), (unsigned long long)sym<uint64_t (*)(P)>("ec_rn50_plan_hash")(h));
    const size_t ws = sym<size_t (*)(P, int)>("ec_rn50_workspace_bytes")(h, frames);
    const P wsp = fake(ws);
    static const float mean3[3] = {0.485f, 0.456f, 0.406f}, std3[3] = {0.229f, 0.224f, 0.225f};   // read on the host by the u8 entry point
    if (input == "f32")
        rc = sym<int (*)(P, P, int, P, size_t, P, int, P)>("ec_rn50_forward")(h, rgb, frames, wsp, ws, out, chunk, nullptr);
    else if (input == "u8")
        rc = sym<int (*)(P, P, const float*, const float*, int, P, size_t, P, int, P)>("ec_rn50_forward_u8")(h, rgb, mean3, std3, frames, wsp, ws,
                                                                                                            out, chunk, nullptr);
    else if (input == "depth")
        rc = sym<int (*)(P, P, float, float, P, int, P, size_t, P, int, P)>("ec_rn50_forward_depth")(h, rgb, 0.2f, -0.5f, w9, frames, wsp, ws, out,
                                                                                                    chunk, nullptr);
    else if (input == "rgbd") {   // `frames` counts pairs; a workspace of the entry point's own size
        const size_t ws2 = sym<size_t (*)(P, int)>("ec_rn50_rgbd_workspace_bytes")(h, frames);
        rc = sym<int (*)(P, P, int, const float*, const float*, P, float, float, P, int, P, size_t, P, int, P)>("ec_rn50_embed_rgbd")(
            h, rgb, 0, nullptr, nullptr, fake(1u << 30), 0.2f, -0.5f, w9, frames, fake(ws2), ws2, out, chunk, nullptr);
    } else
        rc = -100;
    sym<void (*)(P)>("ec_rn50_destroy")(h);
    return rc;
}

// v: the first 13 ec_policy_cfg fields, then T, N, mode, bf16, reuse, dhf, core, prev_action_dims, prev_action_null, face
static int run_policy(const int* v) {
    typedef void* P;
    typedef uint64_t U;
    const int T = v[13], N = v[14], mode = v[15], bf16 = v[16], reuse = v[17], dhf = v[18], goal_in = v[12], dual = v[11], face = v[22];
    const bool learn_pass = mode == 2, act = (face >= 1 && face <= 4) || face >= 6;
    if (mode < 0 || mode > 2 || (reuse && mode != 0) || (dhf && !learn_pass)) return -100;
    if (face < 0 || face > 7 || (act && (mode != 0 || T != 1))) return -100;
    void* h = nullptr;
    int cfg[32] = {0};                                  // the 15 fields, zero-filled behind them (fields a later header adds read 0)
    memcpy(cfg, v, 13 * sizeof(int));
    cfg[13] = v[20]; cfg[14] = v[21];
    int rc = v[19] ? sym<int (*)(P*, const int*, int, int)>("ec_policy_create_rnn_layers")(&h, cfg, v[19] / 10, v[19] % 10)
                   : sym<int (*)(P*, const int*)>("ec_policy_create")(&h, cfg);
    if (rc) return rc;
    const size_t ws = sym<size_t (*)(P, int, int, int)>("ec_policy_workspace_bytes")(h, T, N, mode != 0);
    printf("W %zu\n", ws);
    const P params = fake(sym<size_t (*)(P)>("ec_policy_flat_size")(h) * 4), feat = fake(1u << 30), feat2 = dual ? fake(1u << 30) : nullptr;
    const P goal = fake(1u << 20), h0 = fake(1u << 24), masks = fake(1u << 20), wsp = fake(ws), hv = fake(1u << 20), hf = fake(1u << 24);
    const P prev = fake(1u << 20), actions = fake(1u << 20), logp = fake(1u << 20), values = fake(1u << 20);
    const bool force = face == 4 || face == 7;
    const P expert = force ? fake(1u << 20) : nullptr, emask = force ? fake(1u << 20) : nullptr;
    const P ids = goal_in > 0 ? nullptr : goal, vec = goal_in > 0 ? goal : nullptr;
    const char* vs = goal_in > 0 ? "_vec" : "";
    auto name = [&](const char* a, const char* b) { return std::string(a) + vs + b; };
    // one call of the face's entry point in EC_POLICY_* mode `md`
    auto fwd = [&](int md) -> int {
        switch (face) {
        case 0:
            return sym<int (*)(P, P, P, P, int, P, P, P, int, int, P, size_t, int, P, P, P)>(goal_in > 0 ? "ec_policy_forward_vec" : "ec_policy_forward2")(
                h, params, feat, feat2, bf16, goal, h0, masks, T, N, wsp, ws, md, hv, hf, nullptr);
        case 1:
            return sym<int (*)(P, P, P, P, int, P, P, P, int, P, size_t, int, P, P, P, P, P, U, U, int, P)>(name("ec_policy_act", "").c_str())(
                h, params, feat, feat2, bf16, goal, h0, masks, N, wsp, ws, md == 2, hv, hf, actions, logp, values, 1, 2, 3, nullptr);
        case 2:
            return sym<int (*)(P, P, P, P, int, P, P, P, int, P, size_t, int, P, P, P, P, P, P)>(name("ec_policy_act", "_greedy").c_str())(
                h, params, feat, feat2, bf16, goal, h0, masks, N, wsp, ws, md == 2, hv, hf, actions, logp, values, nullptr);
        case 3: case 4:
            return sym<int (*)(P, P, P, P, int, P, P, P, P, int, P, size_t, int, P, P, P, P, P, int, U, U, int, P, P, float, P)>("ec_policy_act_ex")(
                h, params, feat, feat2, bf16, ids, vec, h0, masks, N, wsp, ws, md == 2, hv, hf, actions, logp, values, 0, 1, 2, 3, expert, emask,
                force ? 0.25f : 0.f, nullptr);
        case 5:
            return sym<int (*)(P, P, P, P, int, P, P, P, P, P, int, int, P, size_t, int, P, P, P)>("ec_policy_forward_pa")(
                h, params, feat, feat2, bf16, ids, vec, prev, h0, masks, T, N, wsp, ws, md, hv, hf, nullptr);
        default:
            return sym<int (*)(P, P, P, P, int, P, P, P, P, P, int, P, size_t, int, P, P, P, P, P, int, U, U, int, P, P, float, P)>("ec_policy_act_pa")(
                h, params, feat, feat2, bf16, ids, vec, prev, h0, masks, N, wsp, ws, md == 2, hv, hf, actions, logp, values, 0, 1, 2, 3, expert,
                emask, force ? 0.25f : 0.f, nullptr);
        }
    };
    g_log_copies = 1;
    if (reuse) {
        rc = fwd(0 /* EC_POLICY_INFER */);
        printf("B %d\n", rc);
    }
    if (!rc) rc = fwd(reuse ? 2 /* EC_POLICY_INFER_REUSE */ : mode != 0);
    if (learn_pass) {
        printf("F %d\n", rc);
        const P dhv = fake(1u << 20), dhfin = dhf ? fake(1u << 24) : nullptr, grads = fake(sym<size_t (*)(P)>("ec_policy_flat_size")(h) * 4);
        if (!rc)
            rc = sym<int (*)(P, P, P, P, int, P, int, int, P, size_t, P, P, P, P)>("ec_policy_backward2")(h, params, feat, feat2, bf16, masks, T, N, wsp,
                                                                                                        ws, dhv, dhfin, grads, nullptr);
    }
    g_log_copies = 0;
    sym<void (*)(P)>("ec_policy_destroy")(h);
    return rc;
}

// v: embed_in hidden embed_dims num_goals num_sensors k0 k1 k2 num_actions prev_action_dims prev_action_null rnn_type num_layers,
// then T, N, mode, reuse, inplace, act
static int run_pooled(const int* v) {
    typedef void* P;
    const int T = v[13], N = v[14], mode = v[15], reuse = v[16], inplace = v[17], act = v[18];
    const bool learn_pass = mode == 2;
    if (mode < 0 || mode > 2 || (reuse && mode != 0) || (act && (mode != 0 || T != 1))) return -100;
    void* h = nullptr;
    int cfg[13];
    memcpy(cfg, v, sizeof cfg);                         // ec_pooled_cfg: thirteen ints in this order
    int rc = sym<int (*)(P*, const int*)>("ec_policy_create_pooled")(&h, cfg);
    if (rc) return rc;
    const size_t ws = sym<size_t (*)(P, int, int, int)>("ec_policy_workspace_bytes")(h, T, N, mode != 0);
    printf("W %zu\n", ws);
    const P params = fake(sym<size_t (*)(P)>("ec_policy_flat_size")(h) * 4), embed = fake(1u << 30);
    const P goal = v[3] ? fake(1u << 20) : nullptr, sens = v[4] ? fake(1u << 20) : nullptr, prev = v[9] ? fake(1u << 20) : nullptr;
    const P h0 = fake(1u << 24), masks = fake(1u << 20), wsp = fake(ws), hv = fake(1u << 24), hf = inplace ? h0 : fake(1u << 24);
    auto fwd_ = sym<int (*)(P, P, P, P, P, P, P, P, int, int, P, size_t, int, P, P, P)>("ec_policy_forward_pooled");
    auto act_ = sym<int (*)(P, P, P, P, P, P, P, P, int, P, size_t, int, P, P, P, P, P, int, uint64_t, uint64_t, int, P, P, float, P)>(
        "ec_policy_act_pooled");
    const P actions = fake(1u << 20), logp = fake(1u << 20);
    auto fwd = [&](P h_, P pr, P e, P g, P sn, P pv, P h0_, P m, int T_, int N_, P w, size_t wb, int md, P hv_, P hf_, P st) {
        if (!act) return fwd_(h_, pr, e, g, sn, pv, h0_, m, T_, N_, w, wb, md, hv_, hf_, st);
        return act_(h_, pr, e, g, sn, pv, h0_, m, N_, w, wb, md == 2, hv_, hf_, actions, logp, nullptr, 0, 1, 2, 0, nullptr, nullptr, 0.f, st);
    };
    g_log_copies = 1;
    if (reuse) {
        rc = fwd(h, params, embed, goal, sens, prev, h0, masks, T, N, wsp, ws, 0 /* EC_POLICY_INFER */, hv, hf, nullptr);
        printf("B %d\n", rc);
    }
    if (!rc) rc = fwd(h, params, embed, goal, sens, prev, h0, masks, T, N, wsp, ws, reuse ? 2 /* EC_POLICY_INFER_REUSE */ : mode != 0, hv, hf, nullptr);
    if (learn_pass) {
        printf("F %d\n", rc);
        const P dhv = fake(1u << 24), grads = fake(sym<size_t (*)(P)>("ec_policy_flat_size")(h) * 4);
        if (!rc)
            rc = sym<int (*)(P, P, P, P, int, P, int, int, P, size_t, P, P, P, P)>("ec_policy_backward2")(h, params, embed, nullptr, 0, masks, T, N, wsp,
                                                                                                        ws, dhv, nullptr, grads, nullptr);
    }
    g_log_copies = 0;
    sym<void (*)(P)>("ec_policy_destroy")(h);
    return rc;
}

// v: the nine ec_two_view_cfg fields (in_channels spatial hidden attn_hidden num_actions prev_action_dims prev_action_null rnn_type
// num_layers), then T, N, mode, reuse, inplace, act
static int run_two_view(const int* v) {
    typedef void* P;
    const int T = v[9], N = v[10], mode = v[11], reuse = v[12], inplace = v[13], act = v[14];
    const bool learn_pass = mode == 2;
    if (mode < 0 || mode > 2 || (reuse && mode != 0) || act < 0 || act > 2 || (act && (mode != 0 || T != 1))) return -100;
    void* h = nullptr;
    int cfg[9];
    memcpy(cfg, v, sizeof cfg);                         // ec_two_view_cfg: nine ints in this order
    int rc = sym<int (*)(P*, const int*)>("ec_policy_create_two_view")(&h, cfg);
    if (rc) return rc;
    const size_t ws = sym<size_t (*)(P, int, int, int)>("ec_policy_workspace_bytes")(h, T, N, mode != 0);
    printf("W %zu\n", ws);
    const P params = fake(sym<size_t (*)(P)>("ec_policy_flat_size")(h) * 4), u = fake(1u << 30), w = fake(1u << 30);
    const P prev = v[5] ? fake(1u << 20) : nullptr;
    const P h0 = fake(1u << 24), masks = fake(1u << 20), wsp = fake(ws), hv = fake(1u << 24), hf = inplace ? h0 : fake(1u << 24);
    const P actions = fake(1u << 20), logp = fake(1u << 20), expert = act == 2 ? fake(1u << 20) : nullptr, emask = act == 2 ? fake(1u << 20) : nullptr;
    auto fwd = [&](int md) -> int {
        if (!act)
            return sym<int (*)(P, P, P, P, P, P, P, int, int, P, size_t, int, P, P, P)>("ec_policy_forward_two_view")(
                h, params, u, w, prev, h0, masks, T, N, wsp, ws, md, hv, hf, nullptr);
        return sym<int (*)(P, P, P, P, P, P, P, int, P, size_t, int, P, P, P, P, P, int, uint64_t, uint64_t, int, P, P, float, P)>(
            "ec_policy_act_two_view")(h, params, u, w, prev, h0, masks, N, wsp, ws, md == 2, hv, hf, actions, logp, nullptr, 0, 1, 2, 3, expert,
                                      emask, act == 2 ? 0.25f : 0.f, nullptr);
    };
    g_log_copies = 1;
    if (reuse) {
        rc = fwd(0 /* EC_POLICY_INFER */);
        printf("B %d\n", rc);
    }
    if (!rc) rc = fwd(reuse ? 2 /* EC_POLICY_INFER_REUSE */ : mode != 0);
    if (learn_pass) {
        printf("F %d\n", rc);
        const P dhv = fake(1u << 24), grads = fake(sym<size_t (*)(P)>("ec_policy_flat_size")(h) * 4);
        if (!rc)
            rc = sym<int (*)(P, P, P, P, int, P, int, int, P, size_t, P, P, P, P)>("ec_policy_backward2")(h, params, u, w, 1, masks, T, N, wsp, ws, dhv,
                                                                                                        nullptr, grads, nullptr);
    }
    g_log_copies = 0;
    sym<void (*)(P)>("ec_policy_destroy")(h);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: launch_log LIB [--args N | --args-of SUBSTR N [INDEX] ...] < commands\n"); return 2; }
    if (argc >= 4 && !strcmp(argv[2], "--args")) g_dumps.push_back({"conv_igemm", 0, atoi(argv[3])});
    for (int i = 2; i + 2 < argc && !strcmp(argv[i], "--args-of"); i += 3) {
        g_dumps.push_back({argv[i + 1], 0, atoi(argv[i + 2])});
        if (i + 3 < argc && strcmp(argv[i + 3], "--args-of")) g_dumps.back().index = atoi(argv[i++ + 3]);
    }
    g_lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!g_lib) { fprintf(stderr, "launch_log: %s\n", dlerror()); return 2; }
    {
        std::vector<std::string> names;
        for (auto& k : g_kernels) names.push_back(k.second);
        for (auto& n : names) printf("K %s\n", n.c_str());
    }
    typedef void* P;
    const P in = fake(1), w = fake(1), bias = fake(1), resb = fake(1), out = fake(1);
    static const float kMean3[3] = {0.485f, 0.456f, 0.406f}, kStd3[3] = {0.229f, 0.224f, 0.225f};   // read on the host by the u8 entry points
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        std::istringstream ss(line);
        std::string cmd;
        if (!(ss >> cmd)) continue;
        line[strcspn(line, "\n")] = 0;
        printf("C %s\n", line);
        int v[24] = {0}, n = 0, rc = -100;
        std::string kind;
        if (cmd == "trunk" || cmd == "tower") ss >> kind;
        const int nmax = cmd == "policy" ? 23 : cmd == "pooled" ? 19 : cmd == "twoview" ? 15 : cmd == "f32" ? 18 : cmd == "tower" ? 9 : 10;
        while (n < nmax && ss >> v[n]) ++n;
        std::string input;
        if (cmd == "tower" && n == 9 && ss >> input) {
            rc = run_tower(kind, v, input);
        } else if (cmd == "policy" && n >= 18 && n <= 23 && n != 21) {
            rc = run_policy(v);
        } else if (cmd == "pooled" && n == 19) {
            rc = run_pooled(v);
        } else if (cmd == "twoview" && n == 15) {
            rc = run_two_view(v);
        } else if (cmd == "conv" && n == 10) {
            const P r = v[8] ? resb : nullptr;
            if (v[9] == 0)
                rc = sym<int (*)(P, P, P, P, P, int, int, int, int, int, int, int, int, P)>("ec_conv_bf16")(
                    in, w, bias, r, out, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], nullptr);
            else
                rc = sym<int (*)(P, P, P, P, P, int, int, int, int, int, int, int, int, int, P)>("ec_conv_bf16_ld")(
                    in, w, bias, r, out, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[9], nullptr);
        } else if (cmd == "s2" && n == 8) {
            rc = sym<int (*)(P, P, P, P, P, int, int, int, int, int, int, int, P)>("ec_conv_bf16_s2")(
                in, w, bias, v[7] ? resb : nullptr, out, v[0], v[1], v[2], v[3], v[4], v[5], v[6], nullptr);
        } else if (cmd == "gemm" && n == 5) {
            rc = sym<int (*)(P, P, P, P, P, int, int, int, int, P)>("ec_gemm_bf16")(in, w, bias, v[4] ? resb : nullptr, out, v[0], v[1],
                                                                                   v[2], v[3], nullptr);
        } else if (cmd == "x3" && n == 4) {
            rc = sym<int (*)(P, P, P, P, long, int, int, int, P)>("ec_gemm_bf16a_x3")(in, w, bias, out, (long)v[0], v[1], v[2], v[3], nullptr);
        } else if (cmd == "f32" && n == 18) {
            const P a_ = (P)((uintptr_t)in + (uintptr_t)v[16]), b_ = (P)((uintptr_t)w + (uintptr_t)v[17]);
            rc = sym<int (*)(P, P, P, int, int, int, long, long, long, long, int, int, P, P, P, int, P, P, int, P)>("ec_gemm_f32")(
                a_, b_, out, v[0], v[1], v[2], (long)v[3], (long)v[4], (long)v[5], (long)v[6], v[7], v[8], v[9] ? bias : nullptr,
                v[10] ? bias : nullptr, v[11] ? resb : nullptr, v[12], v[13] ? resb : nullptr, v[14] ? bias : nullptr, v[15], nullptr);
        } else if (cmd == "pair" && n == 6) {
            rc = sym<int (*)(P, P, P, P, P, P, P, P, P, P, P, long, int, int, int, P)>("ec_conv1x1_pair_bf16")(
                in, w, bias, v[4] ? in : nullptr, v[4] ? w : nullptr, v[4] ? bias : nullptr, v[5] ? resb : nullptr, out, w, bias, out, (long)v[0],
                v[1], v[2], v[3], nullptr);
        } else if (cmd == "rebuild" && n == 4) {
            rc = sym<int (*)(P, P, P, P, P, P, P, P, P, P, P, P, P, long, int, int, int, P)>("ec_conv1x1_pair_rebuild_bf16")(
                in, w, bias, in, w, bias, in, w, bias, out, w, bias, out, (long)v[0], v[1], v[2], v[3], nullptr);
        } else if (cmd == "pairpool" && n == 7) {
            rc = sym<int (*)(P, P, P, P, P, P, P, P, P, int, int, int, int, int, int, P)>("ec_conv1x1_pair_pool_bf16")(
                in, w, bias, resb, v[6] ? out : nullptr, out, w, bias, out, v[0], v[1], v[2], v[3], v[4], v[5], nullptr);
        } else if (cmd == "img" && n == 5) {
            rc = sym<int (*)(P, P, int, P)>("ec_conv3x3_img_pack")(w, w, v[2], nullptr);
            if (!rc)
                rc = sym<int (*)(P, P, P, P, int, int, int, int, int, int, P)>("ec_conv3x3_img_bf16_ld")(in, w, bias, out, v[0], v[1], v[1], v[2], v[3],
                                                                                                       v[4] ? v[4] : v[2], nullptr);
        } else if (cmd == "bneck23" && n == 4) {
            rc = sym<int (*)(P, P, P, int, P)>("ec_bneck_pack_weights")(w, w, w, v[3], nullptr);
            if (!rc)
                rc = sym<int (*)(P, P, P, P, P, P, int, int, int, int, P)>("ec_bneck_conv23_bf16")(in, w, bias, bias, resb, out, v[0], v[1], v[2], v[3],
                                                                                                 nullptr);
        } else if (cmd == "bneck123" && n == 4) {
            rc = sym<int (*)(P, P, P, P, int, P)>("ec_bneck3_pack_weights")(w, w, w, w, v[3], nullptr);
            if (!rc)
                rc = sym<int (*)(P, P, P, P, P, P, int, int, int, int, P)>("ec_bneck_conv123_bf16")(in, w, bias, bias, bias, out, v[0], v[1], v[2], v[3],
                                                                                                  nullptr);
        } else if (cmd == "tail" && n == 6) {
            rc = sym<int (*)(P, P, P, P, P, int, int, int, int, int, int, P)>("ec_basic_tail_s2_bf16")(in, resb, w, bias, out, v[0], v[1], v[2], v[3],
                                                                                                     v[4], v[5], nullptr);
        } else if (cmd == "stem" && n == 5) {
            if (v[4])
                rc = sym<int (*)(P, const float*, const float*, P, P, P, int, int, int, int, P)>("ec_stem_conv1_u8")(in, kMean3, kStd3, w, bias, out, v[0],
                                                                                                                    v[1], v[2], v[3], nullptr);
            else
                rc = sym<int (*)(P, P, P, P, int, int, int, int, P)>("ec_stem_conv1")(in, w, bias, out, v[0], v[1], v[2], v[3], nullptr);
        } else if (cmd == "stem7" && n == 4) {
            rc = sym<int (*)(P, int, const float*, const float*, P, P, P, int, int, int, P)>("ec_stem7_pool")(in, v[3], kMean3, kStd3, w, bias, out, v[0],
                                                                                                             v[1], v[2], nullptr);
        } else if (cmd == "dstem" && n == 4) {
            rc = sym<int (*)(P, float, float, P, P, P, int, int, int, int, P)>("ec_stem_conv1_depth")(in, 4.f, -2.f, w, bias, out, v[0], v[1], v[2], v[3],
                                                                                                     nullptr);
        } else if (cmd == "avgpool" && n == 5) {
            if (v[4] == 0)
                rc = sym<int (*)(P, P, int, int, int, int, P)>("ec_avgpool2_bf16")(in, out, v[0], v[1], v[2], v[3], nullptr);
            else
                rc = sym<int (*)(P, P, int, int, int, int, int, P)>("ec_avgpool2_bf16_ld")(in, out, v[0], v[1], v[2], v[3], v[4], nullptr);
        } else if (cmd == "tonchw" && n == 3) {
            rc = sym<int (*)(P, P, int, int, int, P)>("ec_nhwc_bf16_to_nchw_f32")(in, out, v[0], v[1], v[2], nullptr);
        } else if (cmd == "tonhwc" && n == 3) {
            rc = sym<int (*)(P, P, int, int, int, P, P)>("ec_nchw_f32_to_nhwc_bf16")(in, out, v[0], v[1], v[2], resb, nullptr);
        } else if (cmd == "mean" && n == 3) {
            rc = sym<int (*)(P, P, int, int, int, P)>("ec_spatial_mean_bf16")(in, out, v[0], v[1], v[2], nullptr);
        } else if (cmd == "trunk" && n == 2) {
            rc = run_trunk(kind, v[0], v[1]);
        } else {
            fprintf(stderr, "launch_log: bad command: %s\n", line);
            return 2;
        }
        printf("R %d\n", rc);
    }
    return 0;
}
