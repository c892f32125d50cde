// ResNet trunk executor: CLIP ModifiedResNet (stem + layer1..4, attnpool detached), torchvision ResNet-50, ResNet-18 / 34.
//
// Replaces `clip_features = clip_model(clip_input)` with `clip_model.attnpool = nn.Identity()`
// (primitive_probing/generate_data/thor_image_features.py:59-67,109) == [U] allenact_plugins/clip_plugin ClipResNetEmbedder.forward.
//
// The plan is derived from the architecture ([U] openai/CLIP clip/model.py ModifiedResNet.__init__/_make_layer, Bottleneck)
// before the first launch, in three steps:
//   slots  walk_arch(): geometry, buffers and the weight / bias offsets of every conv, in the order ec_amd.h documents
//   forms  block_form(): what a block runs as (plain convs, a boundary pair, a K-concatenated tail, a fused bottleneck, ...): a
//          function of the architecture, the block's position and ec_config() -- and of the NEXT block's form, equally static
//   ops    plan_bottleneck() / plan_basic() append the block's ops in that form.  A fused op carries as its PARTS the plain convs
//          it stands for, made by mk_conv() like every other conv, with their buffers and slots
// rn50_run() is a straight line of launches over five ping-pong NHWC bf16 buffers in the caller's workspace: one runner per op
// kind, whose route function picks the launch for this chunk's frame count; every fallback runs the op's parts through run_conv().
// CLIP's anti-aliased stride (3x3 conv at full resolution, then AvgPool2d(2)) is fused into the 3x3 conv's epilogue; the
// residual add + ReLU is fused into conv3's epilogue.
#include <stdlib.h>

#include <new>
#include <vector>

#include "common.h"

// (common.h includes include/ec_amd.h, which declares the conv_bneck.hip entry points used below)

namespace {

enum OpKind { OP_STEM1, OP_CONV, OP_POOL, OP_PAIR, OP_BNECK, OP_STEM7, OP_BTAIL, OP_CAT, OP_CONV_POOLOUT };   // (values: ec_rn50_plan_hash)

// buffers: 0 = X (block input / output), 1,2 = temporaries, 3 = identity path, 4 = Y; and
constexpr int BUF_NONE = -1, BUF_IN = -2, BUF_OUT = -3;   // no operand; the caller's frames; the caller's feature tensor

struct Slot { size_t w = 0, b = 0; };   // one conv's element offsets into w_bf16 / bias

// One plain convolution: an op of its own (OP_CONV) or a part of a fused op.  run_conv() is the only code that launches one.
struct Conv {
    int src, dst, res;        // buffer ids
    int H, W, Cin, Cout, ks, pool, act;
    int stride;               // 2 = torchvision's strided conv (ec_conv_bf16_s2); H, W are the INPUT dims
    Slot at;
    int ldo = 0, ocol = 0;    // writing a column block of a wider tensor: row stride (0 = dense) and first column (elements)
    int img_max = 0;          // > 0: a 3x3 conv that launches of up to this many frames run on the image-resident kernel (img3_max_frames)
    size_t wimg_off = 0;      // ... from its streaming-order weights at this offset (elements) into wbneck
};

// [a | b] . [Wa | Wb]^T + (ba + bb): two convs as ONE GEMM over the concatenated K axis, from weights laid side by side in wbneck
// and the summed bias in bias_cat (pack_plan_weights)
struct Cat { Slot a, b; int Ka, Kb; size_t w_off = 0, b_off = 0; };   // (offsets: elements into wbneck / bias_cat)

struct Op {
    OpKind kind;
    // OP_STEM1 / OP_STEM7: the stem conv on the caller's frames.  OP_CONV: the conv.  OP_CONV_POOLOUT: a block's conv3.
    // OP_CAT: the GEMM over the concatenated K axis (geometry and buffers; its weights are `cat`'s)
    Conv c;
    // OP_POOL: AvgPool2d(2) of src [H, W, C] into a column block of dst (ldo 0: dense).  pool_of: skipped when the previous
    // block's OP_CONV_POOLOUT wrote it already.  pd: where that op's pooled copy goes (buffer, row stride, column)
    struct { int src, dst, H, W, C, ldo, ocol, pool_of; } pl;
    struct { int dst, ld, col; } pd;
    // The parts of a fused op --
    // OP_PAIR (conv_pair.hip): y = relu(c3 [+ ds] [+ c3.res]) -> c3.dst, z = relu(next_c1(y)) -> next_c1.dst, the NEXT block's conv1
    // OP_BNECK (conv_bneck.hip): conv2 + conv3 + identity + ReLU of one Bottleneck; with fold_c1 its conv1 too
    // OP_BTAIL (conv_basic.hip): a BasicBlock's stride-2 tail, relu(c2(conv1's output) + ds(block input)), as one `cat` GEMM
    Conv c1, c2, c3, ds, next_c1;
    bool fold_ds;        // OP_PAIR: the block's downsample conv is folded in as a second K operand (its output is never materialised)
    bool no_y;           // OP_PAIR: y is not stored: the next boundary launch rebuilds it (ec_rn50_set_l1_rebuild)
    bool rebuild;        // OP_PAIR: ... and this is that launch (conv_pair_rebuild.hip): the identity is relu(id_c3 + id_ds), the
    Conv id_c3, id_ds;   //          PREVIOUS block's conv3 and folded downsample conv, recomputed from their inputs
    int pooled_dst;      // OP_PAIR at the layer-1 -> layer-2 boundary: buffer for AvgPool2d(2)(y), the next block's downsample input; or BUF_NONE
    bool fold_c1;        // OP_BNECK: the whole block in one launch
    size_t wpack_off;    // OP_BNECK: its streaming-order weights in wbneck (ec_bneck_pack_weights / ec_bneck3_pack_weights)
    Cat cat;             // OP_CAT, OP_BTAIL
};

}  // namespace

struct ec_rn50 {
    int width, res, out_c, out_sp;
    int tv = 0;                   // 1: torchvision ResNet (7x7 stem + max-pool, stride inside conv2 / the downsample conv): ec_rn50tv_create;
                                  // 2: torchvision BasicBlock ResNet (ResNet-18 / 34): ec_tvresnet_basic_create
    std::vector<Op> ops;
    size_t max_elems_per_frame;   // largest activation (bf16 elements) per frame
    const float* stem_w;
    const uint16_t* w;
    const float* bias;
    size_t n_w, n_b;
    int conv8_min_tiles = 0;      // 0 = library default (ec_rn50_set_conv8_min_tiles)
    int layers4[4] = {0, 0, 0, 0};
    int l1_rebuild = 0;           // layer 1's block-0 output is rebuilt, not stored (ec_rn50_set_l1_rebuild)
    uint16_t* wbneck = nullptr;   // weights the plan's launches read in their own layout: Cat::w_off, Op::wpack_off, Conv::wimg_off
    float* bias_cat = nullptr;    // summed biases of the K-concatenated GEMMs (Cat::b_off)
    ~ec_rn50() {
        if (wbneck) (void)hipFree(wbneck);
        if (bias_cat) (void)hipFree(bias_cat);
    }
};

namespace {
constexpr int NBUF = 5;
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

enum TowerKind { CLIP = 0, TV_BOTTLENECK = 1, TV_BASIC = 2 };   // (== ec_rn50::tv)

struct Blk {
    int li, planes, inplanes, stride;
    int R, Ro;                // resolution of the block's input / output
    int x, out;               // buffers of the block's input / output (ping-pong between 0 and 4; the last block writes BUF_OUT)
    int y;                    // the ping-pong buffer opposite x (== out but for the last block): free until the block's last launch
    bool ds, last_of_layer;
    Slot c1, c2, c3, dsc;     // (a BasicBlock has no c3; dsc only where the block downsamples)
};
struct Arch {
    TowerKind kind; int width, R1;   // R1: resolution behind the stem
    bool l1_rebuild;                 // block 0's output is never stored: its input lives in that buffer instead (walk_arch)
    Slot stem[3], total; std::vector<Blk> B;
};

// The architecture before any op is planned, in the order ec_amd.h documents: stem convs (CLIP: conv1's weights are passed apart,
// fp32; the 7x7 stem: all of them), then per block conv1, conv2, conv3, [downsample] (BasicBlock: conv1, conv2, [downsample])
Arch walk_arch(TowerKind kind, int width, int sc, const int* layers4, int R, bool l1_rebuild = false) {
    Arch a{kind, width, R, l1_rebuild};
    Slot& at = a.total;
    auto take = [&](size_t Cout, size_t K) { const Slot s = at; at.w += Cout * K; at.b += Cout; return s; };
    a.stem[0] = take(kind == CLIP ? sc : width, 0);
    if (kind == CLIP) { a.stem[1] = take(sc, (size_t)9 * sc); a.stem[2] = take(width, (size_t)9 * sc); }
    const int expansion = kind == TV_BASIC ? 1 : 4;
    int inplanes = width, x = 0;
    for (int li = 0; li < 4; ++li)
        for (int b = 0; b < layers4[li]; ++b) {
            Blk k{li, width << li, inplanes, (b == 0 && li > 0) ? 2 : 1};
            const size_t p = k.planes, in = inplanes;
            k.ds = k.stride > 1 || inplanes != k.planes * expansion;
            k.last_of_layer = b + 1 == layers4[li];
            k.R = R; k.Ro = R / k.stride;
            k.x = x; k.y = k.out = (x == 0) ? 4 : 0;
            k.c1 = take(p, kind == TV_BASIC ? 9 * in : in);
            k.c2 = take(p, 9 * p);
            if (kind != TV_BASIC) k.c3 = take(4 * p, p);
            if (k.ds) k.dsc = take(expansion * p, in);
            a.B.push_back(k);
            x = k.y; inplanes = k.planes * expansion; R = k.Ro;
        }
    if (!a.B.empty()) a.B.back().out = BUF_OUT;
    // Block 1's boundary launch reads block 0's input across the whole tensor while it writes its own output: the two must not
    // share a buffer.  Block 0's output buffer holds nothing, so the stem writes the block input there.
    if (l1_rebuild && !a.B.empty()) a.B[0].x = a.B[0].y;
    return a;
}

// The image-resident K-split 3x3 kernel (conv3x3_img_kernel) instead of conv_igemm: up to how many frames per launch (0: not this conv).
// The three limits: a fused bottleneck's conv2 run alone (14x14x256) while its (image, slice) workgroups fit one round, 8 * frames <= 256;
// the un-pooled 7x7x512 convs, two rounds of workgroups at most; layer4.0's pooled 14x14x512 conv2 (two channel chunks, 16 slices per
// image: one round of workgroups) -- at 32 frames it ties with conv_igemm (47.6 vs 46.6 us).  (The kernel has no residual input: a
// BasicBlock's conv2 stays on conv_igemm.)
int img3_max_frames(const Conv& c, bool bneck_conv2 = false) {
    if (!ec_config().rn50_img3 || c.ks != 3) return 0;
    if (bneck_conv2) return 32;
    if (c.Cin != 512 || c.Cout != 512 || c.res >= 0) return 0;
    return !c.pool && c.H == 7 && c.W == 7 ? 64 : c.pool && c.H == 14 && c.W == 14 ? 16 : 0;
}

Conv mk_conv(int src, int dst, int res, int H, int W, int Cin, int Cout, int ks, int pool, int act, Slot at, int stride = 1) {
    Conv c{src, dst, res, H, W, Cin, Cout, ks, pool, act, stride, at};
    c.img_max = img3_max_frames(c);
    return c;
}

struct Plan {   // what the planners append to
    std::vector<Op>& ops;
    size_t mx = 0;   // largest activation per frame so far
    void track(int H, int W, int C) { mx = std::max(mx, (size_t)H * W * C); }
    void push(const Op& o, int H, int W, int C) { ops.push_back(o); track(H, W, C); }
    void conv(const Conv& c) {
        Op o{OP_CONV, c};
        const int half = (c.pool || c.stride == 2) ? 2 : 1;
        push(o, c.H / half, c.W / half, c.Cout);
    }
    void pool(int src, int dst, int R, int C, int ldo, int ocol, bool pool_of) {
        Op o{OP_POOL};
        o.pl = {src, dst, R, R, C, ldo, ocol, pool_of};
        push(o, R / 2, R / 2, ldo ? ldo : C);
    }
};

// What the previous block's boundary launch (OP_PAIR) already produced for this block: the buffer of its conv1 output and
// (layer-1 -> layer-2) of the pooled block input for the downsample path
struct Given { int c1_buf = BUF_NONE, pooled_in = BUF_NONE; };

enum Form {
    F_PLAIN,        // conv1, conv2, [pool,] [downsample conv,] conv3
    F_POOLOUT,      // ... whose conv3 may also emit the pooled copy of its output for the next block's F_CAT
    F_PAIR1,        // layer 1: conv3 (+ the block-0 downsample conv) + identity + ReLU chained into the next block's conv1, one launch
    F_PAIR1_POOL,   // ... that also emits the pooled block output (the next block pools its input)
    F_PAIR2,        // layer 2: conv3 + identity + ReLU and the next block's conv1 in one launch
    F_CAT,          // stride-2 block of layers 3-4: conv3 | downsample conv as one GEMM over the concatenated K axis
    F_BNECK         // conv2 + conv3 (+ conv1) + identity + ReLU in one launch per image
};

Form block_form(const Arch& a, size_t i) {
    const Blk& k = a.B[i];
    const Blk* nx = i + 1 < a.B.size() ? &a.B[i + 1] : nullptr;
    const auto& cfg = ec_config();
    // Layer-1 block boundaries (56x56, bandwidth-bound 1x1 convs) run as ONE fused launch per boundary:
    // conv3 (+ the block-0 downsample conv) + identity + ReLU, chained in registers into the next block's conv1.
    const bool fuse = cfg.rn50_fuse != 0 && a.width == 64 && (a.R1 % 8) == 0;   // K = 64, N = 256; 32-pixel tiles divide R*R
    // boundary fusion applies to every block of layer 1 that is followed by a 1x1 conv1 on its output
    // (downsample + a 128-wide conv1 exceeds the LDS)
    if (fuse && k.li == 0 && nx && nx->li <= 1 && (!k.ds || (k.inplanes == k.planes && !k.last_of_layer)))
        return (a.kind == CLIP && k.last_of_layer && !k.ds) ? F_PAIR1_POOL : F_PAIR1;
    // Stride-2 blocks of layers 3-4 (CLIP: AvgPool2d(2) after conv2 and in front of the downsample conv): the pooled conv2
    // output [M, planes] and the pooled block input [M, inplanes] are laid side by side, and
    //   relu(conv3(c2) + b3 + downsample(xp) + bd) == relu([c2 | xp] . [W3 | Wd]^T + (b3 + bd))
    // is ONE GEMM with K = planes + inplanes: the downsample output (M x 4 planes) is never written or re-read, one
    // launch less, and the sum is rounded to bf16 once instead of twice.  (layer 2's first block gets its pooled
    // input from the layer-1 boundary launch and chains conv3 into the next conv1: left as is.)
    if (k.ds && a.kind == CLIP && k.stride > 1 && k.li >= 2 && cfg.rn50_dscat && (k.planes % 8) == 0) return F_CAT;
    // Layer-2 block boundaries (28x28, 128 -> 512 -> 128): conv3 + identity + ReLU and the next block's conv1 in
    // one launch with the weights in registers (conv_pair.hip, layer-2 geometry).
    if (fuse && k.li == 1 && k.planes == 128 && !k.last_of_layer) return F_PAIR2;
    // Bottleneck-level fusion (conv_bneck.hip): conv2 + conv3 + identity + ReLU of layer3.1 .. layer3.5 in one launch, one
    // workgroup per image with the 14 x 14 x 256 map resident in LDS
    if (cfg.rn50_bneck > 0 && !k.ds && k.stride == 1 && k.planes == 256 && k.Ro == 14) return F_BNECK;
    // layer 2's last conv3 (128 -> 512 + identity @28x28) can emit the pooled copy the next block's concatenated operand needs
    // (conv1x1_regw_kernel<.., PL>); whether it did is known per launch (run_conv_poolout)
    if (cfg.rn50_poolout && k.planes == 128 && nx && block_form(a, i + 1) == F_CAT) return F_POOLOUT;
    return F_PLAIN;
}

Given plan_bottleneck(Plan& p, const Arch& a, size_t i, Given g) {
    const Blk& k = a.B[i];
    const Blk* nx = i + 1 < a.B.size() ? &a.B[i + 1] : nullptr;
    const Form f = block_form(a, i);
    const bool tv = a.kind != CLIP, c1_given = g.c1_buf != BUF_NONE;
    const int planes = k.planes, inplanes = k.inplanes, R = k.R, Ro = k.Ro, x = k.x, c1_buf = c1_given ? g.c1_buf : 1;
    // EC_RN50_BNECK3 (default 1): conv1 too -- the whole Bottleneck is ONE launch (bneck23_kernel<.., F1>), conv1's output never leaves the LDS
    const bool fold_c1 = f == F_BNECK && ec_config().rn50_bneck3 && !c1_given;
    const Conv c1 = mk_conv(x, 1, BUF_NONE, R, R, inplanes, planes, 1, 0, EC_ACT_RELU, k.c1);
    // conv2: torchvision strides inside the 3x3 conv itself, CLIP pools behind it
    Conv c2 = tv && k.stride > 1 ? mk_conv(c1_buf, 2, BUF_NONE, R, R, planes, planes, 3, 0, EC_ACT_RELU, k.c2, 2)
                                 : mk_conv(c1_buf, 2, BUF_NONE, R, R, planes, planes, 3, k.stride > 1 ? 1 : 0, EC_ACT_RELU, k.c2);
    if (!c1_given && !fold_c1) p.conv(c1);
    Op o{};
    if (f == F_BNECK) {   // launches below EC_RN50_BNECK frames run the parts (bneck_route)
        o.kind = OP_BNECK; o.fold_c1 = fold_c1;
        o.c1 = c1; o.c2 = c2; o.c2.img_max = img3_max_frames(c2, true);
        o.c3 = mk_conv(2, k.out, x, Ro, Ro, planes, planes * 4, 1, 0, EC_ACT_RELU, k.c3);
        p.push(o, Ro, Ro, planes * 4);
        return Given{};
    }
    if (f == F_PAIR1 || f == F_PAIR1_POOL) {
        // l1_rebuild: block 0's boundary stores no y; block 1's rebuilds it from block 0's conv2 output (buffer 2) and input, so
        // block 1's conv2 writes buffer 3 (free inside layer 1 until the layer-1 -> layer-2 boundary writes the pooled copy)
        const bool rb0 = a.l1_rebuild && i == 0, rb1 = a.l1_rebuild && i == 1;
        if (rb1) c2.dst = 3;
        p.conv(c2);
        o.kind = OP_PAIR;
        o.c3 = mk_conv(c2.dst, k.out, k.ds || rb1 ? BUF_NONE : x, R, R, planes, planes * 4, 1, 0, EC_ACT_RELU, k.c3);
        o.fold_ds = k.ds;   // block 0: the downsample conv (x -> 256) is folded in as a second K = 64 operand
        if (k.ds) o.ds = mk_conv(x, BUF_NONE, BUF_NONE, R, R, inplanes, planes * 4, 1, 0, EC_ACT_NONE, k.dsc);
        o.no_y = rb0;
        if (rb1) {
            const Blk& b0 = a.B[0];
            o.rebuild = true;
            o.id_c3 = mk_conv(2, BUF_NONE, BUF_NONE, R, R, b0.planes, b0.planes * 4, 1, 0, EC_ACT_RELU, b0.c3);
            o.id_ds = mk_conv(b0.x, BUF_NONE, BUF_NONE, R, R, b0.inplanes, b0.planes * 4, 1, 0, EC_ACT_NONE, b0.dsc);
        }
        o.next_c1 = mk_conv(k.out, 1, BUF_NONE, R, R, planes * 4, nx->planes, 1, 0, EC_ACT_RELU, nx->c1);
        o.pooled_dst = f == F_PAIR1_POOL ? 3 : BUF_NONE;
        if (f == F_PAIR1_POOL) p.track(R / 2, R / 2, planes * 4);
        p.push(o, R, R, planes * 4);
        return Given{1, o.pooled_dst};
    }
    if (f == F_CAT) {
        const int Kc = planes + inplanes;
        // The concatenated operand lives in buffer 3 (free in layers 3-4), not in buffer 2: the conv3 that PRODUCES this block's
        // input reads its own conv2 output from buffer 2 and may write the pooled columns in the same launch (F_POOLOUT).
        const int cat = 3;
        c2.dst = cat; c2.ldo = Kc;   // conv2 (+ pool) -> columns [0, planes)
        p.conv(c2);
        p.pool(x, cat, R, inplanes, Kc, planes, i > 0 && block_form(a, i - 1) == F_POOLOUT);   // pooled block input -> columns [planes, Kc)
        o.kind = OP_CAT;
        o.c = mk_conv(cat, k.out, BUF_NONE, Ro, Ro, Kc, planes * 4, 1, 0, EC_ACT_RELU, Slot{});
        o.cat = Cat{k.c3, k.dsc, planes, inplanes};
        p.push(o, Ro, Ro, planes * 4);
        return Given{};
    }
    // F_PLAIN, F_POOLOUT, F_PAIR2: conv2, the downsample path, conv3.  (The weights are laid out conv1, conv2, conv3, downsample;
    // the downsample conv has to run BEFORE conv3, which consumes its output as the residual.)
    p.conv(c2);
    int idt = x;
    if (k.ds) {
        int dsrc = x, ddst = 3;
        if (tv) {
            // torchvision: downsample = Conv2d(1x1, stride) + BatchNorm2d straight on the block input
        } else if (k.stride > 1 && g.pooled_in != BUF_NONE) {   // pooled input came with the previous boundary launch;
            dsrc = g.pooled_in;                                  // buffer 1 (this block's conv1 output) is free after conv2
            ddst = 1;
        } else if (k.stride > 1) {
            // the pooled block input goes to the block's OUTPUT buffer y (free until conv3 writes it), not to the
            // conv1 / conv2 temporaries
            p.pool(x, k.y, R, inplanes, 0, 0, false);
            dsrc = k.y;
        }
        p.conv(tv && k.stride > 1 ? mk_conv(dsrc, ddst, BUF_NONE, R, R, inplanes, planes * 4, 1, 0, EC_ACT_NONE, k.dsc, 2)
                                  : mk_conv(dsrc, ddst, BUF_NONE, Ro, Ro, inplanes, planes * 4, 1, 0, EC_ACT_NONE, k.dsc));
        idt = ddst;
    }
    const Conv c3 = mk_conv(2, k.out, idt, Ro, Ro, planes, planes * 4, 1, 0, EC_ACT_RELU, k.c3);
    if (f == F_PLAIN) { p.conv(c3); return Given{}; }
    if (f == F_PAIR2) {   // frame counts whose row count is not a multiple of 32 run the two convs separately (run_pair)
        o.kind = OP_PAIR;
        o.c3 = c3;
        o.next_c1 = mk_conv(k.out, idt == 1 ? 3 : 1, BUF_NONE, Ro, Ro, planes * 4, planes, 1, 0, EC_ACT_RELU, nx->c1);   // (block 0 with a pooled input keeps its identity in buffer 1)
        o.pooled_dst = BUF_NONE;
    } else {   // F_POOLOUT
        o.kind = OP_CONV_POOLOUT;
        o.c = c3;
        o.pd = {3, nx->planes + nx->inplanes, nx->planes};   // the next block's concatenated operand, behind its conv2 columns
    }
    p.push(o, Ro, Ro, planes * 4);
    return f == F_PAIR2 ? Given{o.next_c1.dst, BUF_NONE} : Given{};
}

// torchvision BasicBlock: conv1: 3x3 + ReLU (stride 2 in the first block of layers 2-4: ec_conv_bf16_s2)
//   conv2: stride-1 blocks  3x3 + identity + ReLU (ec_conv_bf16 with a residual)
//          transition blocks 3x3 over conv1's output + the 1x1 stride-2 downsample conv of the block input + ReLU as ONE
//                            K-concatenated GEMM (OP_BTAIL, conv_basic.hip)
// Buffers: the block input / output ping-pong between 0 and 4, conv1's output goes to 1; buffer 3 holds the downsample
// output of a transition tail that runs as two launches (btail_fused).
void plan_basic(Plan& p, const Blk& k) {
    const int planes = k.planes, Ro = k.Ro;
    p.conv(mk_conv(k.x, 1, BUF_NONE, k.R, k.R, k.inplanes, planes, 3, 0, EC_ACT_RELU, k.c1, k.stride));
    if (!k.ds) {   // conv2 + identity + ReLU
        p.conv(mk_conv(1, k.out, k.x, Ro, Ro, planes, planes, 3, 0, EC_ACT_RELU, k.c2));
        return;
    }
    Op o{};   // (torchvision downsamples exactly where it strides)
    o.kind = OP_BTAIL;
    o.ds = mk_conv(k.x, 3, BUF_NONE, k.R, k.R, k.inplanes, planes, 1, 0, EC_ACT_NONE, k.dsc, 2);
    o.c2 = mk_conv(1, k.out, 3, Ro, Ro, planes, planes, 3, 0, EC_ACT_RELU, k.c2);
    o.cat = Cat{k.c2, k.dsc, 9 * planes, k.inplanes};
    p.push(o, Ro, Ro, planes);
}

// Weights the plan's fused / K-concatenated / image-resident launches read in their own layout (device copies owned by the handle)
size_t cat_n(const Op& o) { return (size_t)(o.kind == OP_CAT ? o.c.Cout : o.c2.Cout); }

// offsets: the concatenated GEMMs ([Cout][Ka + Kb] weights, summed bias), then per fused bottleneck one packed block (its conv2
// comes first in it: what the image-resident kernel reads when conv2 runs alone) and the image-resident 3x3 convs.
// A function of the op list alone: a plan rebuilt for the same tower (ec_rn50_set_l1_rebuild) finds its weights where they are.
void plan_offsets(std::vector<Op>& ops, size_t& tot, size_t& btot) {
    tot = btot = 0;
    for (Op& o : ops)
        if (o.kind == OP_CAT || o.kind == OP_BTAIL) {
            o.cat.w_off = tot; tot += cat_n(o) * (size_t)(o.cat.Ka + o.cat.Kb);
            o.cat.b_off = btot; btot += cat_n(o);
        }
    for (Op& o : ops) {
        if (o.kind == OP_BNECK) { o.wpack_off = o.c2.wimg_off = tot; tot += ec_bneck3_packed_elems(o.c2.Cin); }   // (room for conv1 too)
        if (o.kind == OP_CONV && o.c.img_max) { o.c.wimg_off = tot; tot += (size_t)o.c.Cout * 9 * o.c.Cin; }
    }
}

int pack_plan_weights(ec_rn50* h) {
    size_t tot = 0, btot = 0;
    plan_offsets(h->ops, tot, btot);
    if (btot && hipMalloc(&h->bias_cat, btot * sizeof(float)) != hipSuccess) { h->bias_cat = nullptr; return EC_ERR_LAUNCH; }
    if (!tot) return EC_OK;
    if (hipMalloc(&h->wbneck, tot * sizeof(uint16_t)) != hipSuccess) { h->wbneck = nullptr; return EC_ERR_LAUNCH; }
    auto pack_cat = [&](const Cat& c, size_t N) -> int {
        const size_t K = (size_t)c.Ka + c.Kb;
        uint16_t* wc = h->wbneck + c.w_off;
        if (hipMemcpy2D(wc, K * 2, h->w + c.a.w, (size_t)c.Ka * 2, (size_t)c.Ka * 2, N, hipMemcpyDeviceToDevice) != hipSuccess ||
            hipMemcpy2D(wc + c.Ka, K * 2, h->w + c.b.w, (size_t)c.Kb * 2, (size_t)c.Kb * 2, N, hipMemcpyDeviceToDevice) != hipSuccess) return EC_ERR_LAUNCH;
        std::vector<float> ba(N), bb(N);
        if (hipMemcpy(ba.data(), h->bias + c.a.b, N * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(bb.data(), h->bias + c.b.b, N * 4, hipMemcpyDeviceToHost) != hipSuccess) return EC_ERR_LAUNCH;
        for (size_t i = 0; i < N; ++i) ba[i] += bb[i];
        return hipMemcpy(h->bias_cat + c.b_off, ba.data(), N * 4, hipMemcpyHostToDevice) != hipSuccess ? EC_ERR_LAUNCH : EC_OK;
    };
    for (const Op& o : h->ops) {
        int rc = EC_OK;
        if (o.kind == OP_CAT || o.kind == OP_BTAIL) rc = pack_cat(o.cat, cat_n(o));
        else if (o.kind == OP_BNECK)
            rc = o.fold_c1 ? ec_bneck3_pack_weights(h->w + o.c1.at.w, h->w + o.c2.at.w, h->w + o.c3.at.w, h->wbneck + o.wpack_off, o.c2.Cin, nullptr)
                           : ec_bneck_pack_weights(h->w + o.c2.at.w, h->w + o.c3.at.w, h->wbneck + o.wpack_off, o.c2.Cin, nullptr);
        else if (o.kind == OP_CONV && o.c.img_max) rc = ec_conv3x3_img_pack(h->w + o.c.at.w, h->wbneck + o.c.wimg_off, o.c.Cin, nullptr);
        if (rc != EC_OK) return EC_ERR_LAUNCH;
    }
    (void)hipStreamSynchronize(nullptr);
    return EC_OK;
}

// stem channels: width/2, rounded up to the 32-channel granule of the conv kernels (RN50x16: 48 -> 64; the
// packer zero-pads the weights, so the padded channels are exactly 0 after ReLU and contribute nothing)
int stem_channels(int width) { return (width / 2 + 31) / 32 * 32; }

// The op list of a tower, stem first; -> the largest activation per frame (bf16 elements)
size_t plan_tower(std::vector<Op>& ops, const Arch& a, int res) {
    ops.clear();
    Plan p{ops};
    const int width = a.width, sc = stem_channels(width);
    const int x0 = a.B.empty() ? BUF_OUT : a.B[0].x;   // the stem's output is the first block's input
    if (a.kind == CLIP) {   // conv1 strides by 2 itself: frame -> buffer 1 at R x R x sc
        const int R = res / 2;
        p.push(Op{OP_STEM1, mk_conv(BUF_IN, 1, BUF_NONE, res, res, 3, sc, 3, 0, EC_ACT_RELU, a.stem[0])}, R, R, sc);
        p.conv(mk_conv(1, 2, BUF_NONE, R, R, sc, sc, 3, 0, EC_ACT_RELU, a.stem[1]));
        p.conv(mk_conv(2, x0, BUF_NONE, R, R, sc, width, 3, 1, EC_ACT_RELU, a.stem[2]));   // + fused AvgPool2d(2)
    } else {   // conv1 7x7 s2 + bn1 + relu + maxpool 3x3 s2 in one launch: frame -> buffer 0 at R1 x R1 x 64
        p.push(Op{OP_STEM7, mk_conv(BUF_IN, x0, BUF_NONE, res, res, 3, width, 7, 0, EC_ACT_RELU, a.stem[0])}, a.R1, a.R1, width);
    }
    Given g;
    for (size_t i = 0; i < a.B.size(); ++i)
        if (a.kind == TV_BASIC) plan_basic(p, a.B[i]);
        else g = plan_bottleneck(p, a, i, g);
    return p.mx;
}

// ec_rn50_set_l1_rebuild: a CLIP tower whose layer1.0 boundary folds the downsample conv and whose layer1.1 boundary is a plain
// fused pair too (not the pooled one: layer 1 has a third block)
bool l1_rebuild_ok(const Arch& a) {
    return a.kind == CLIP && a.B.size() >= 3 && a.B[0].ds && block_form(a, 0) == F_PAIR1 && block_form(a, 1) == F_PAIR1;
}

// The one builder: the towers differ in their stem and in their block planner
int rn50_build(ec_rn50_t** out, TowerKind kind, int width, const int* layers4, int input_resolution, const void* stem_w,
               const void* w_bf16, size_t n_w, const float* bias, size_t n_bias) {
    if (!out || !layers4 || !stem_w || !w_bf16 || !bias) return EC_ERR_ARG;
    if (width % 32 != 0 || width < 32 || input_resolution % 32 != 0) return EC_ERR_SHAPE;
    if (kind == TV_BASIC && (input_resolution < 32 || layers4[0] < 1 || layers4[1] < 1 || layers4[2] < 1 || layers4[3] < 1)) return EC_ERR_SHAPE;
    const int res = input_resolution;
    const Arch a = walk_arch(kind, width, stem_channels(width), layers4, res / 4);
    if (n_w != a.total.w || n_bias != a.total.b) return EC_ERR_SHAPE;
    ec_rn50* h = new (std::nothrow) ec_rn50();
    if (!h) return EC_ERR_ALLOC;
    h->width = width; h->res = res; h->tv = kind;
    std::copy(layers4, layers4 + 4, h->layers4);
    h->stem_w = (const float*)stem_w; h->w = (const uint16_t*)w_bf16; h->bias = bias;
    h->n_w = a.total.w; h->n_b = a.total.b;
    h->max_elems_per_frame = plan_tower(h->ops, a, res);
    h->out_c = a.B.empty() ? width : a.B.back().planes * (kind == TV_BASIC ? 1 : 4);
    h->out_sp = a.B.empty() ? a.R1 : a.B.back().Ro;
    const int rc = pack_plan_weights(h);
    if (rc != EC_OK) { delete h; return rc; }
    *out = h;
    return EC_OK;
}
}  // namespace

extern "C" int ec_rn50_create(ec_rn50_t** out, int width, const int* layers4, int input_resolution, const float* stem_w_f32,
                              const void* w_bf16, size_t n_w, const float* bias, size_t n_bias) {
    return rn50_build(out, CLIP, width, layers4, input_resolution, stem_w_f32, w_bf16, n_w, bias, n_bias);
}

// torchvision ResNet (v1.5) trunk == Sequential(*list(resnet50.children())[:-2])
// (primitive_probing/generate_data/thor_image_features.py:46-49): the same executor and, for every stride-1 conv, the same
// launches as the CLIP trunk; the stem is ONE launch (7x7 s2 conv + bn + relu + 3x3 s2 max-pool, stem7.hip) and the first
// block of layers 2-4 strides inside its 3x3 conv and its 1x1 downsample conv (ec_conv_bf16_s2) instead of pooling.
extern "C" int ec_rn50tv_create(ec_rn50_t** out, const int* layers4, int input_resolution, const void* stem_w_bf16,
                                const void* w_bf16, size_t n_w, const float* bias, size_t n_bias) {
    return rn50_build(out, TV_BOTTLENECK, 64, layers4, input_resolution, stem_w_bf16, w_bf16, n_w, bias, n_bias);
}

// torchvision BasicBlock ResNet (ResNet-18: 2,2,2,2 / ResNet-34: 3,4,6,3) without avgpool / fc, behind the same handle:
// the 7x7 stem launch of ec_rn50tv_create, then plan_basic() per block
extern "C" int ec_tvresnet_basic_create(ec_rn50_t** out, const int* layers4, int input_resolution, const void* stem_w_bf16,
                                        const void* w_bf16, size_t n_w, const float* bias, size_t n_bias) {
    return rn50_build(out, TV_BASIC, 64, layers4, input_resolution, stem_w_bf16, w_bf16, n_w, bias, n_bias);
}

extern "C" void ec_rn50_destroy(ec_rn50_t* h) { delete h; }
extern "C" int ec_rn50_out_channels(const ec_rn50_t* h) { return h ? h->out_c : 0; }
extern "C" int ec_rn50_out_spatial(const ec_rn50_t* h) { return h ? h->out_sp : 0; }
extern "C" int ec_rn50_num_ops(const ec_rn50_t* h) { return h ? (int)h->ops.size() : 0; }

// FNV-1a over the launch plan (op kinds, shapes, buffer routing) and the library version: what a PMC traffic
// summary under profiles/ was measured on.  bench.py refuses a summary whose hash differs (stale evidence).
extern "C" uint64_t ec_rn50_plan_hash(const ec_rn50_t* h) {
    if (!h) return 0;
    uint64_t x = 1469598103934665603ull;
    auto mix = [&](long v) {
        for (int i = 0; i < 8; ++i) { x ^= (uint64_t)((v >> (8 * i)) & 0xff); x *= 1099511628211ull; }
    };
    mix(ec_version()); mix((long)ec_config_hash());
    mix(h->width); mix(h->res); mix(h->conv8_min_tiles); mix(h->tv);
    if (h->l1_rebuild) mix(h->l1_rebuild);   // (only while on: a default handle keeps the key its summaries were measured on)
    for (const Op& o : h->ops) {
        // The 24 values per op and their order are FROZEN (the flat op record of the versions the summaries under profiles/ were
        // measured on): a plan that launches the same kernels must keep its key.  0 kind, 1 src, 2 dst, 3 res, 4 H, 5 W, 6 Cin, 7 Cout,
        // 8 ks, 9 pool, 10 act, 11 stride, 12 second source, 13 second dst, 14 second width / first K share, 15 pooled dst, 16 conv1
        // folded, 17 ldo, 18 ocol, 19 concatenated K, 20-22 pooled-output buffer, row stride, column, 23 pool_of
        const Conv& c = o.kind == OP_PAIR || o.kind == OP_BNECK ? o.c3 : o.kind == OP_BTAIL ? o.c2 : o.c;
        long f[24] = {o.kind, c.src, c.dst, c.res, c.H, c.W, c.Cin, c.Cout, c.ks, c.pool, c.act, c.stride, -1, -1, 0, -1, 0, c.ldo, c.ocol, 0, -1, 0, 0, 0};
        if (o.kind == OP_POOL) {
            const long p[12] = {OP_POOL, o.pl.src, o.pl.dst, -1, o.pl.H, o.pl.W, o.pl.C, o.pl.C, 0, 0, 0, 1};
            std::copy(p, p + 12, f);
            f[17] = o.pl.ldo; f[18] = o.pl.ocol; f[23] = o.pl.pool_of;
        }
        if (o.kind == OP_PAIR) { f[12] = o.fold_ds ? o.ds.src : -1; f[13] = o.next_c1.dst; f[14] = o.next_c1.Cout; f[15] = o.pooled_dst; }
        if (o.kind == OP_BNECK) { f[1] = o.c2.src; f[8] = 3; f[16] = o.fold_c1; }
        if (o.kind == OP_BTAIL) { f[3] = -1; f[6] = o.cat.Ka + o.cat.Kb; f[12] = o.ds.src; f[14] = o.cat.Ka; f[19] = 1; }
        if (o.kind == OP_CAT) { f[0] = OP_CONV; f[14] = o.cat.Ka; f[19] = 1; }
        if (o.kind == OP_CONV_POOLOUT) { f[0] = OP_CONV; f[20] = o.pd.dst; f[21] = o.pd.ld; f[22] = o.pd.col; }
        for (long v : f) mix(v);
    }
    return x;
}

extern "C" int ec_rn50_set_conv8_min_tiles(ec_rn50_t* h, int n) {
    if (!h) return EC_ERR_ARG;
    h->conv8_min_tiles = n > 0 ? n : 0;
    return EC_OK;
}

// The plan is rebuilt from the architecture, as at creation.  The packed weights stay where they are: their offsets are a function
// of the op kinds (plan_offsets), and layer 1 has no packed weights.
extern "C" int ec_rn50_set_l1_rebuild(ec_rn50_t* h, int on) {
    if (!h) return EC_ERR_ARG;
    const Arch a = walk_arch((TowerKind)h->tv, h->width, stem_channels(h->width), h->layers4, h->res / 4, on != 0);
    if (!l1_rebuild_ok(a)) return EC_ERR_UNSUPPORTED;
    if ((on != 0) == (h->l1_rebuild != 0)) return EC_OK;
    std::vector<Op> ops;
    const size_t mx = plan_tower(ops, a, h->res);
    size_t tot = 0, btot = 0;
    plan_offsets(ops, tot, btot);
    if (mx != h->max_elems_per_frame) return EC_ERR_UNSUPPORTED;   // (cannot happen: the ops' shapes are those of the default plan)
    h->ops.swap(ops);
    h->l1_rebuild = on != 0;
    return EC_OK;
}

extern "C" size_t ec_rn50_workspace_bytes(const ec_rn50_t* h, int batch) {
    if (!h || batch <= 0) return 0;
    return NBUF * align_up(h->max_elems_per_frame * 2 * (size_t)batch, 256);
}

namespace {
// What the frames are: the stem op is the only one that looks at them.
struct FrameIn {
    enum Kind { F32, U8, DEPTH, RGBD } kind;
    const void* p;                 // F32: fp32 [B,R,R,3]; U8: uint8 [B,R,R,3]; DEPTH: fp32 [B,R,R] (one channel); RGBD: the RGB frames
    const float *mean3, *std3;     // uint8 RGB frames: host pointers
    float scale, shift;            // DEPTH, RGBD: value = depth * scale + shift
    const float* stem_w9;          // DEPTH, RGBD: the stem weights summed over the input channels, f32 [9][stem channels]
    const float* depth = nullptr;  // RGBD: the depth frames fp32 [B,R,R] that pair with p, frame by frame
    bool rgb_u8 = false;           // RGBD: p is uint8
    bool u8() const { return kind == U8 || (kind == RGBD && rgb_u8); }
};
struct Run {   // one chunk of frames on its way through the plan
    const ec_rn50* h;
    const FrameIn& in;
    const void* frames;    // this chunk's RGB frames, or NULL
    const float* depth;    // this chunk's depth frames, or NULL.  With both, the chunk is nb / 2 RGB frames, then nb / 2 depth frames
    int nb;                // frames on their way through the plan
    unsigned char* base;   // the workspace: NBUF buffers of bufsz bytes
    size_t bufsz;
    void* out;             // where the last op writes: this chunk's rows of the caller's feature tensor, or of the RGB-D pass's map region
    hipStream_t stream;
    bool pooled_emitted;   // the last OP_CONV_POOLOUT wrote the pooled copy of its output: the OP_POOL marked pool_of is skipped
    void* buf(int id) const { return id == BUF_OUT ? out : base + (size_t)id * bufsz; }
    const void* opt(int id) const { return id == BUF_NONE ? nullptr : buf(id); }
};

// Every plain conv, op or part: the strided kernel, the image-resident 3x3 kernel for small launches (img3_max_frames), conv_igemm
int run_conv(const Run& r, const Conv& c) {
    const ec_rn50* h = r.h;
    if (c.stride == 2)
        return ec_conv_bf16_s2(r.buf(c.src), h->w + c.at.w, h->bias + c.at.b, r.opt(c.res), r.buf(c.dst), r.nb, c.H, c.W, c.Cin, c.Cout, c.ks,
                               c.act, r.stream);
    uint16_t* dst = (uint16_t*)r.buf(c.dst) + c.ocol;
    if (r.nb <= c.img_max)
        return ec_conv3x3_img_bf16_ld(r.buf(c.src), h->wbneck + c.wimg_off, h->bias + c.at.b, dst, r.nb, c.H, c.W, c.Cin, c.pool,
                                      c.ldo ? c.ldo : c.Cin, r.stream);
    return ec_conv_bf16_ld(r.buf(c.src), h->w + c.at.w, h->bias + c.at.b, r.opt(c.res), dst, r.nb, c.H, c.W, c.Cin, c.Cout, c.ks, c.pool, c.act,
                           c.ldo ? c.ldo : c.Cout, r.stream);
}

int run_stem(const Run& r, const Op& o) {
    const FrameIn& in = r.in;
    const Conv& c = o.c;
    const float* bias = r.h->bias + c.at.b;
    if (o.kind == OP_STEM7)
        return ec_stem7_pool(r.frames, in.u8() ? 1 : 0, in.mean3, in.std3, r.h->stem_w, bias, r.buf(c.dst), r.nb, c.H, c.W, r.stream);
    // RGB frames fill the destination's first rows, depth frames the rows behind them: a joint RGB-D chunk is two launches into one
    // buffer, and every later op sees nb frames of the same tensor
    const int n_rgb = !r.frames ? 0 : r.depth ? r.nb / 2 : r.nb;
    int rc = EC_OK;
    if (n_rgb && in.u8())
        rc = ec_stem_conv1_u8((const uint8_t*)r.frames, in.mean3, in.std3, r.h->stem_w, bias, r.buf(c.dst), n_rgb, c.H, c.W, c.Cout, r.stream);
    else if (n_rgb)
        rc = ec_stem_conv1((const float*)r.frames, r.h->stem_w, bias, r.buf(c.dst), n_rgb, c.H, c.W, c.Cout, r.stream);
    if (rc != EC_OK || !r.depth) return rc;
    const size_t frame_out = (size_t)((c.H - 1) / 2 + 1) * ((c.W - 1) / 2 + 1) * c.Cout;   // (the stem conv strides by 2, pad 1)
    return ec_stem_conv1_depth(r.depth, in.scale, in.shift, in.stem_w9, bias, (uint16_t*)r.buf(c.dst) + (size_t)n_rgb * frame_out, r.nb - n_rgb,
                               c.H, c.W, c.Cout, r.stream);
}

int run_pool(Run& r, const Op& o) {
    const auto& p = o.pl;
    if (p.pool_of && r.pooled_emitted) { r.pooled_emitted = false; return EC_OK; }
    if (p.ldo) return ec_avgpool2_bf16_ld(r.buf(p.src), (uint16_t*)r.buf(p.dst) + p.ocol, r.nb, p.H, p.W, p.C, p.ldo, r.stream);
    return ec_avgpool2_bf16(r.buf(p.src), r.buf(p.dst), r.nb, p.H, p.W, p.C, r.stream);
}

// conv3 that may also emit AvgPool2d(2) of its output.  The launch itself is the route function: conv1x1_regw_kernel<.., PL> takes an
// even frame count of at least 42 and returns EC_ERR_SHAPE otherwise; the plain conv3 runs then, and the OP_POOL marked pool_of pools
int run_conv_poolout(Run& r, const Op& o) {
    const Conv& c = o.c;
    const int rc = ec_conv1x1_regw_pool(r.buf(c.src), r.h->w + c.at.w, r.h->bias + c.at.b, r.buf(c.res), r.buf(c.dst),
                                        (uint16_t*)r.buf(o.pd.dst) + o.pd.col, r.nb, c.H, c.W, c.Cin, c.Cout, c.act, o.pd.ld, r.stream);
    if (rc == EC_OK) r.pooled_emitted = true;
    return rc == EC_ERR_SHAPE ? run_conv(r, c) : rc;
}

int run_cat(const Run& r, const Op& o) {   // conv3 | downsample conv over the concatenated K axis
    const Conv& c = o.c;
    return ec_conv_bf16_ld(r.buf(c.src), r.h->wbneck + o.cat.w_off, r.h->bias_cat + o.cat.b_off, nullptr, r.buf(c.dst), r.nb, c.H, c.W, c.Cin,
                           c.Cout, 1, 0, c.act, c.Cout, r.stream);
}

// The boundary launch is its own route function too: EC_ERR_SHAPE for a row count that is no multiple of its tile (e.g. an odd number
// of 28x28 frames), and the two convs run separately.  (With the downsample conv folded in, the pooled copy or the rebuilt identity
// there is no such route: those forms are planned only where 32-pixel tiles divide the frame.)
int run_pair(const Run& r, const Op& o) {
    const ec_rn50* h = r.h;
    const Conv &c3 = o.c3, &c1 = o.next_c1;
    if (o.pooled_dst != BUF_NONE)
        // (the full-resolution block output is dead here: the next block reads c1.dst and pooled_dst only)
        return ec_conv1x1_pair_pool_bf16(r.buf(c3.src), h->w + c3.at.w, h->bias + c3.at.b, r.buf(c3.res), nullptr, r.buf(o.pooled_dst),
                                         h->w + c1.at.w, h->bias + c1.at.b, r.buf(c1.dst), r.nb, c3.H, c3.W, c3.Cin, c3.Cout, c1.Cout, r.stream);
    if (o.rebuild)   // the identity is the previous block's output, rebuilt from that block's conv2 output and input
        return ec_conv1x1_pair_rebuild_bf16(r.buf(c3.src), h->w + c3.at.w, h->bias + c3.at.b, r.buf(o.id_c3.src), h->w + o.id_c3.at.w,
                                            h->bias + o.id_c3.at.b, r.buf(o.id_ds.src), h->w + o.id_ds.at.w, h->bias + o.id_ds.at.b,
                                            r.buf(c3.dst), h->w + c1.at.w, h->bias + c1.at.b, r.buf(c1.dst), (long)r.nb * c3.H * c3.W,
                                            c3.Cin, c3.Cout, c1.Cout, r.stream);
    int rc = ec_conv1x1_pair_bf16(r.buf(c3.src), h->w + c3.at.w, h->bias + c3.at.b, o.fold_ds ? r.buf(o.ds.src) : nullptr,
                                  o.fold_ds ? h->w + o.ds.at.w : nullptr, o.fold_ds ? h->bias + o.ds.at.b : nullptr, r.opt(c3.res),
                                  o.no_y ? nullptr : r.buf(c3.dst), h->w + c1.at.w, h->bias + c1.at.b, r.buf(c1.dst), (long)r.nb * c3.H * c3.W, c3.Cin, c3.Cout,
                                  c1.Cout, r.stream);
    if (rc == EC_ERR_SHAPE && !o.fold_ds) {
        rc = run_conv(r, c3);
        if (rc == EC_OK) rc = run_conv(r, c1);
    }
    return rc;
}

// Launches below EC_RN50_BNECK frames run the convs separately: a workgroup per image only fills the chip from ~128 images on.
bool bneck_fused(int nb) { return nb >= ec_config().rn50_bneck; }

int run_bneck(const Run& r, const Op& o) {
    const ec_rn50* h = r.h;
    const Conv &c1 = o.c1, &c2 = o.c2, &c3 = o.c3;
    if (bneck_fused(r.nb) && o.fold_c1)
        return ec_bneck_conv123_bf16(r.buf(c3.res), h->wbneck + o.wpack_off, h->bias + c1.at.b, h->bias + c2.at.b, h->bias + c3.at.b,
                                     r.buf(c3.dst), r.nb, c3.H, c3.W, c2.Cin, r.stream);
    if (bneck_fused(r.nb))
        return ec_bneck_conv23_bf16(r.buf(c2.src), h->wbneck + o.wpack_off, h->bias + c2.at.b, h->bias + c3.at.b, r.buf(c3.res),
                                    r.buf(c3.dst), r.nb, c3.H, c3.W, c2.Cin, r.stream);
    // (buffer 1 = conv1's, buffer 2 = conv2's output, as in the unfused plan; conv2 on the image-resident kernel while it fits one round)
    int rc = o.fold_c1 ? run_conv(r, c1) : EC_OK;
    if (rc == EC_OK) rc = run_conv(r, c2);
    return rc == EC_OK ? run_conv(r, c3) : rc;
}

// The one-launch tail where it measured faster than the two launches (profiles/basic_tail_ab.txt): layer2.0 at every frame count,
// layer3.0 up to 32 frames.  Deeper-K / larger launches: the downsample conv into buffer 3, then conv2 with it as the residual
// (the 8-wave and ring instances of conv_igemm win there).
bool btail_fused(const Op& o, int nb) { return o.c2.Cout <= 128 || (o.c2.Cout <= 256 && nb <= 32); }

int run_btail(const Run& r, const Op& o) {
    const Conv &c2 = o.c2, &ds = o.ds;
    if (btail_fused(o, r.nb))
        return ec_basic_tail_s2_bf16(r.buf(c2.src), r.buf(ds.src), r.h->wbneck + o.cat.w_off, r.h->bias_cat + o.cat.b_off, r.buf(c2.dst), r.nb,
                                     c2.H, c2.W, c2.Cin, ds.Cin, c2.Cout, r.stream);
    const int rc = run_conv(r, ds);
    return rc == EC_OK ? run_conv(r, c2) : rc;
}

// An RGB-D chunk of nb pairs: one pass of the plan at 2 nb frames (EC_RGBD_JOINT, default 1), or two passes at nb frames, RGB then depth.
// The only place that chooses, per chunk.  Measured at 32 / 64 / 128 pairs (profiles/rgbd_pooled_bench.txt) the joint pass is
// 14-26 % faster than two forwards, two pools and an add, so no pair count is sent to the composed route.
bool rgbd_joint(int /*pairs*/) { return ec_config().rgbd_joint != 0; }

// feat: bf16 [batch, S, S, C], the last op's output -- or, for FrameIn::RGBD, f32 [batch, C]: the mean over the pixels of the RGB
// frame's map plus the depth frame's (ec_spatial_mean_pair_bf16), `batch` and `chunk` counting PAIRS; the maps of a chunk live in
// the workspace behind the NBUF buffers (ec_rn50_rgbd_workspace_bytes).
int rn50_run(const ec_rn50_t* h, const FrameIn& in, int batch, void* workspace, size_t ws_bytes, void* feat, int chunk,
             ec_stream_t stream_main) {
    const bool rgbd = in.kind == FrameIn::RGBD;
    if (!h || !in.p || !workspace || !feat || (rgbd && !in.depth)) return EC_ERR_ARG;
    if (batch <= 0) return EC_ERR_SHAPE;
    if ((in.kind == FrameIn::DEPTH || rgbd) && (h->ops.empty() || h->ops.front().kind != OP_STEM1))
        return EC_ERR_UNSUPPORTED;   // the 7x7 stem of the torchvision towers has no one-channel kernel
    if (chunk <= 0 || chunk > batch) chunk = batch;
    const int per = rgbd ? 2 : 1;   // frames in the buffers per unit of `chunk`
    {   // the conv kernels address activations through 32-bit buffer descriptors (< 2 GiB per tensor)
        const long maxc = ((1L << 31) - 1) / (long)(h->max_elems_per_frame * 2) / per;
        if (chunk > maxc) chunk = (int)(maxc > 0 ? maxc : 1);
    }
    if (ws_bytes < (rgbd ? ec_rn50_rgbd_workspace_bytes(h, chunk) : ec_rn50_workspace_bytes(h, chunk))) return EC_ERR_WORKSPACE;
    const ec_min_tiles_scope mint_scope(h->conv8_min_tiles);   // this handle's dispatch threshold, for this call only
    const size_t bufsz = align_up(h->max_elems_per_frame * 2 * (size_t)chunk * per, 256);
    // bytes per frame: a depth frame has ONE channel
    const size_t frame_bytes = (size_t)h->res * h->res * (in.kind == FrameIn::DEPTH ? 1 : 3) * (in.u8() ? 1 : 4);
    const size_t out_stride = (size_t)h->out_sp * h->out_sp * h->out_c;
    const hipStream_t stream = (hipStream_t)stream_main;
    auto pass = [&](Run r) -> int {   // the one walk over the plan
        for (const Op& o : h->ops) {
            int rc;
            switch (o.kind) {
                case OP_STEM1:
                case OP_STEM7: rc = run_stem(r, o); break;
                case OP_POOL: rc = run_pool(r, o); break;
                case OP_PAIR: rc = run_pair(r, o); break;
                case OP_BNECK: rc = run_bneck(r, o); break;
                case OP_BTAIL: rc = run_btail(r, o); break;
                case OP_CAT: rc = run_cat(r, o); break;
                case OP_CONV_POOLOUT: rc = run_conv_poolout(r, o); break;
                default: rc = run_conv(r, o.c);
            }
            if (rc != EC_OK) return rc;
        }
        return EC_OK;
    };
    unsigned char* const base = (unsigned char*)workspace;
    for (int b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = std::min(chunk, batch - b0);
        const void* frames = (const unsigned char*)in.p + (size_t)b0 * frame_bytes;
        int rc;
        if (!rgbd) {
            const bool d = in.kind == FrameIn::DEPTH;
            rc = pass(Run{h, in, d ? nullptr : frames, d ? (const float*)frames : nullptr, nb, base, bufsz,
                          (uint16_t*)feat + (size_t)b0 * out_stride, stream, false});
        } else {
            const float* dep = in.depth + (size_t)b0 * h->res * h->res;
            uint16_t* map = (uint16_t*)(base + NBUF * bufsz);   // [2 nb, S, S, C]: the RGB frames' maps, then the depth frames'
            if (rgbd_joint(nb)) {
                rc = pass(Run{h, in, frames, dep, 2 * nb, base, bufsz, map, stream, false});
            } else {
                rc = pass(Run{h, in, frames, nullptr, nb, base, bufsz, map, stream, false});
                if (rc == EC_OK) rc = pass(Run{h, in, nullptr, dep, nb, base, bufsz, map + (size_t)nb * out_stride, stream, false});
            }
            if (rc == EC_OK)
                rc = ec_spatial_mean_pair_bf16(map, map + (size_t)nb * out_stride, (float*)feat + (size_t)b0 * h->out_c, nb,
                                               h->out_sp * h->out_sp, h->out_c, stream_main);
        }
        if (rc != EC_OK) return rc;
    }
    return EC_OK;
}
}  // namespace

extern "C" size_t ec_rn50_rgbd_workspace_bytes(const ec_rn50_t* h, int pairs) {
    if (!h || pairs <= 0) return 0;
    const size_t map = (size_t)2 * pairs * h->out_sp * h->out_sp * h->out_c * sizeof(uint16_t);
    return ec_rn50_workspace_bytes(h, 2 * pairs) + align_up(map, 256);
}

// [U] ResNetCLIPEncoder.forward with rgb and depth (habitat branch): the trunk on both frames of every pair, the two maps summed and
// average-pooled to ONE vector.  Both towers read the same weights, so a chunk of nb pairs is one pass of the plan at 2 nb frames.
extern "C" int ec_rn50_embed_rgbd(const ec_rn50_t* h, const void* rgb, int rgb_u8, const float* h_mean3, const float* h_std3,
                                  const float* depth, float scale, float shift, const float* stem_w9, int pairs, void* workspace,
                                  size_t ws_bytes, float* embed, int chunk, ec_stream_t stream) {
    if (!depth || !stem_w9 || (rgb_u8 && (!h_mean3 || !h_std3))) return EC_ERR_ARG;
    FrameIn in{FrameIn::RGBD, rgb, h_mean3, h_std3, scale, shift, stem_w9};
    in.depth = depth;
    in.rgb_u8 = rgb_u8 != 0;
    return rn50_run(h, in, pairs, workspace, ws_bytes, embed, chunk, stream);
}

extern "C" int ec_rn50_forward(const ec_rn50_t* h, const float* rgb, int batch, void* workspace, size_t ws_bytes,
                               void* feat, int chunk, ec_stream_t stream) {
    return rn50_run(h, FrameIn{FrameIn::F32, rgb, nullptr, nullptr, 1.f, 0.f, nullptr}, batch, workspace, ws_bytes, feat, chunk, stream);
}

extern "C" int ec_rn50_forward_u8(const ec_rn50_t* h, const uint8_t* rgb_u8, const float* h_mean3, const float* h_std3, int batch,
                                  void* workspace, size_t ws_bytes, void* feat, int chunk, ec_stream_t stream) {
    if (!h_mean3 || !h_std3) return EC_ERR_ARG;
    return rn50_run(h, FrameIn{FrameIn::U8, rgb_u8, h_mean3, h_std3, 1.f, 0.f, nullptr}, batch, workspace, ws_bytes, feat, chunk, stream);
}

// The depth tower of the RGB-D agent: the same plan, OP_STEM1 on the one-channel kernel (stem_depth.hip).  The handle stays
// pointer-only: the folded stem weights come with the call.
extern "C" int ec_rn50_forward_depth(const ec_rn50_t* h, const float* depth, float scale, float shift, const float* stem_w9,
                                     int batch, void* workspace, size_t ws_bytes, void* feat, int chunk, ec_stream_t stream) {
    if (!stem_w9) return EC_ERR_ARG;
    return rn50_run(h, FrameIn{FrameIn::DEPTH, depth, nullptr, nullptr, scale, shift, stem_w9}, batch, workspace, ws_bytes, feat, chunk, stream);
}
