// Host-only planner of the FID Inception network (csrc/inception.hip): the layer table, shape propagation for any input size, the
// activation buffers and their sizes, the channel slice every launch writes, the conv tile per launch and the refusal rules.
// Plain C++17, no HIP: tests/inception_plan_shim.cpp compiles it for the CPU tests.
//
// The network is pytorch-fid's "FID Inception" (the reference's pnpflow/models.py:498-820) in eval mode.  A layer is BasicConv2d:
// bias-free conv, BatchNorm on running statistics (eps 1e-3), ReLU.  Activations are NHWC; a Mixed block's branches write their channel
// slice of the block's output tensor directly (channel offset + total width), so a concatenation is never executed.
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>
#include <utility>
#include <vector>

namespace pf {
namespace inc {

constexpr int INC_SIDE = 299;           // the side the optional bilinear resize produces (models.py:634-638)
constexpr int INC_MIN_SIDE = 75;        // below it Mixed_7a's stride-2 3x3 has no output pixel
constexpr int INC_KC = 16;              // K-chunk of the conv kernel; packed weights pad K = KH*KW*Cin up to a multiple of it
constexpr int INC_CU = 256;             // compute units of an MI355X: the tile rule below fills them once before it takes the larger tile

struct Layer { std::string name; int Cin, Cout, KH, KW, S, PH, PW; };

// conv tiles (MT pixels x NT output channels per 256-thread workgroup; four waves as 2 x 2, each (MT/2) x (NT/2))
enum Tile { T128x128 = 0, T128x64 = 1, T64x128 = 2, T64x64 = 3, NUM_TILES = 4 };
inline int tile_mt(int t) { return (t == T128x128 || t == T128x64) ? 128 : 64; }
inline int tile_nt(int t) { return (t == T128x128 || t == T64x128) ? 128 : 64; }

// NT = 128 only where it pads Cout no further than NT = 64 does (48, 64, 80 -> 128, 192, 320, 448 keep 64); MT = 128 only when the
// launch then still has a workgroup for every compute unit.
inline int choose_tile(long long M, int Cout) {
    const int n128 = (Cout + 127) / 128 * 128, n64 = (Cout + 63) / 64 * 64;
    const int NT = (n128 == n64) ? 128 : 64;
    const long long wg128 = ((M + 127) / 128) * ((Cout + NT - 1) / NT);
    const int MT = wg128 >= INC_CU ? 128 : 64;
    return MT == 128 ? (NT == 128 ? T128x128 : T128x64) : (NT == 128 ? T64x128 : T64x64);
}

enum OpKind { OP_CONV = 0, OP_MAXPOOL_S2 = 1, OP_AVGPOOL_S1 = 2, OP_MAXPOOL_S1 = 3 };
// IN0: resized / normalised NHWC input.  X, Y: block input / output, alternating.  T0, T1: branch intermediates.  P: the pooled block input.
enum Buf { BUF_IN0 = 0, BUF_X = 1, BUF_Y = 2, BUF_T0 = 3, BUF_T1 = 4, BUF_P = 5, NUM_BUFS = 6 };

struct Op {
    int kind = OP_CONV, layer = -1;                  // layer: index into layers() for OP_CONV
    int src = 0, src_off = 0, src_cs = 0;            // buffer, first channel, total channels of the source tensor
    int dst = 0, dst_off = 0, dst_cs = 0;
    int C = 0;                                       // channels read (conv: Cin, pool: the slice width)
    int Hi = 0, Wi = 0, Ho = 0, Wo = 0;
    int tile = -1;
};

struct Slice { std::string branch; int off, len; };
struct Block { std::string name; int width = 0, H = 0, W = 0; std::vector<Slice> slices; };

struct Plan {
    bool ok = false;
    std::string err;
    int B = 0, H0 = 0, W0 = 0;                       // batch and the side the network sees (299 with resize)
    std::vector<Op> ops;
    std::vector<Block> blocks;                       // the eleven Mixed blocks, in order, as far as the plan goes
    std::vector<std::pair<int, int>> sides;          // (H, W) after Conv2d_1a, 2a, 2b, maxpool, 3b, 4a, maxpool, Mixed_6a, Mixed_7a
    size_t buf_floats[NUM_BUFS] = {0, 0, 0, 0, 0, 0};
    int out_buf = 0, out_C = 0, out_H = 0, out_W = 0; // the tensor the requested output block is averaged from
};

inline const std::vector<Layer>& layers() {
    static const std::vector<Layer> L = [] {
        std::vector<Layer> v;
        auto add = [&](const std::string& n, int ci, int co, int kh, int kw, int s, int ph, int pw) { v.push_back({n, ci, co, kh, kw, s, ph, pw}); };
        add("Conv2d_1a_3x3", 3, 32, 3, 3, 2, 0, 0);
        add("Conv2d_2a_3x3", 32, 32, 3, 3, 1, 0, 0);
        add("Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1);
        add("Conv2d_3b_1x1", 64, 80, 1, 1, 1, 0, 0);
        add("Conv2d_4a_3x3", 80, 192, 3, 3, 1, 0, 0);
        const struct { const char* n; int ci, pf; } A[3] = {{"Mixed_5b", 192, 32}, {"Mixed_5c", 256, 64}, {"Mixed_5d", 288, 64}};
        for (const auto& a : A) {
            const std::string p = std::string(a.n) + ".";
            add(p + "branch1x1", a.ci, 64, 1, 1, 1, 0, 0);
            add(p + "branch5x5_1", a.ci, 48, 1, 1, 1, 0, 0);
            add(p + "branch5x5_2", 48, 64, 5, 5, 1, 2, 2);
            add(p + "branch3x3dbl_1", a.ci, 64, 1, 1, 1, 0, 0);
            add(p + "branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1);
            add(p + "branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1);
            add(p + "branch_pool", a.ci, a.pf, 1, 1, 1, 0, 0);
        }
        add("Mixed_6a.branch3x3", 288, 384, 3, 3, 2, 0, 0);
        add("Mixed_6a.branch3x3dbl_1", 288, 64, 1, 1, 1, 0, 0);
        add("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1);
        add("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 3, 2, 0, 0);
        const struct { const char* n; int c7; } Cb[4] = {{"Mixed_6b", 128}, {"Mixed_6c", 160}, {"Mixed_6d", 160}, {"Mixed_6e", 192}};
        for (const auto& c : Cb) {
            const std::string p = std::string(c.n) + ".";
            add(p + "branch1x1", 768, 192, 1, 1, 1, 0, 0);
            add(p + "branch7x7_1", 768, c.c7, 1, 1, 1, 0, 0);
            add(p + "branch7x7_2", c.c7, c.c7, 1, 7, 1, 0, 3);
            add(p + "branch7x7_3", c.c7, 192, 7, 1, 1, 3, 0);
            add(p + "branch7x7dbl_1", 768, c.c7, 1, 1, 1, 0, 0);
            add(p + "branch7x7dbl_2", c.c7, c.c7, 7, 1, 1, 3, 0);
            add(p + "branch7x7dbl_3", c.c7, c.c7, 1, 7, 1, 0, 3);
            add(p + "branch7x7dbl_4", c.c7, c.c7, 7, 1, 1, 3, 0);
            add(p + "branch7x7dbl_5", c.c7, 192, 1, 7, 1, 0, 3);
            add(p + "branch_pool", 768, 192, 1, 1, 1, 0, 0);
        }
        add("Mixed_7a.branch3x3_1", 768, 192, 1, 1, 1, 0, 0);
        add("Mixed_7a.branch3x3_2", 192, 320, 3, 3, 2, 0, 0);
        add("Mixed_7a.branch7x7x3_1", 768, 192, 1, 1, 1, 0, 0);
        add("Mixed_7a.branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3);
        add("Mixed_7a.branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0);
        add("Mixed_7a.branch7x7x3_4", 192, 192, 3, 3, 2, 0, 0);
        const struct { const char* n; int ci; } E[2] = {{"Mixed_7b", 1280}, {"Mixed_7c", 2048}};
        for (const auto& e : E) {
            const std::string p = std::string(e.n) + ".";
            add(p + "branch1x1", e.ci, 320, 1, 1, 1, 0, 0);
            add(p + "branch3x3_1", e.ci, 384, 1, 1, 1, 0, 0);
            add(p + "branch3x3_2a", 384, 384, 1, 3, 1, 0, 1);
            add(p + "branch3x3_2b", 384, 384, 3, 1, 1, 1, 0);
            add(p + "branch3x3dbl_1", e.ci, 448, 1, 1, 1, 0, 0);
            add(p + "branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1);
            add(p + "branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1);
            add(p + "branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0);
            add(p + "branch_pool", e.ci, 192, 1, 1, 1, 0, 0);
        }
        return v;
    }();
    return L;
}

inline int layer_index(const std::string& name) {
    const auto& L = layers();
    for (size_t i = 0; i < L.size(); ++i)
        if (L[i].name == name) return (int)i;
    return -1;
}

inline int conv_out(int in, int k, int s, int p) { return (in + 2 * p - k) / s + 1; }
inline int packed_k(const Layer& l) { return (l.KH * l.KW * l.Cin + INC_KC - 1) / INC_KC * INC_KC; }
inline int block_dims(int output_block) { return output_block == 0 ? 64 : output_block == 1 ? 192 : output_block == 2 ? 768 : 2048; }

// The launches of one forward up to `output_block` (0..3) for B images of H x W.  With resize the network sees 299 x 299 whatever the input;
// without it a side below 75 is refused (Mixed_7a would have no output pixel; the earlier blocks are refused with it so that one rule
// holds for every output block).
inline Plan plan(int B, int H, int W, bool resize, int output_block) {
    Plan p;
    p.B = B;
    if (B <= 0 || H <= 0 || W <= 0) { p.err = "Inception: batch and image sides must be positive"; return p; }
    if (output_block < 0 || output_block > 3) { p.err = "Inception: output block must be 0..3"; return p; }
    if ((long long)B * std::max(H, INC_SIDE) * std::max(W, INC_SIDE) > (1ll << 31) / 64) { p.err = "Inception: batch too large for one forward (split it)"; return p; }
    p.H0 = resize ? INC_SIDE : H; p.W0 = resize ? INC_SIDE : W;
    if (p.H0 < INC_MIN_SIDE || p.W0 < INC_MIN_SIDE) {
        p.err = "Inception: without resize_input an image side below " + std::to_string(INC_MIN_SIDE) + " leaves no pixel for Mixed_7a (got " +
                std::to_string(H) + " x " + std::to_string(W) + ")";
        return p;
    }
    int h = p.H0, w = p.W0;
    auto need = [&](int buf, int hh, int ww, int cs) { p.buf_floats[buf] = std::max(p.buf_floats[buf], (size_t)B * hh * ww * cs); };
    // one conv launch; returns through ho / wo
    auto conv = [&](const std::string& name, int src, int src_cs, int dst, int dst_off, int dst_cs, int hi, int wi, int& ho, int& wo) {
        const int li = layer_index(name);
        const Layer& l = layers()[li];
        Op o; o.kind = OP_CONV; o.layer = li; o.src = src; o.src_off = 0; o.src_cs = src_cs; o.dst = dst; o.dst_off = dst_off; o.dst_cs = dst_cs; o.C = l.Cin;
        o.Hi = hi; o.Wi = wi; o.Ho = ho = conv_out(hi, l.KH, l.S, l.PH); o.Wo = wo = conv_out(wi, l.KW, l.S, l.PW);
        o.tile = choose_tile((long long)B * o.Ho * o.Wo, l.Cout);
        need(dst, o.Ho, o.Wo, dst_cs);
        p.ops.push_back(o);
    };
    auto pool = [&](int kind, int src, int C, int dst, int dst_off, int dst_cs, int hi, int wi, int& ho, int& wo) {
        Op o; o.kind = kind; o.src = src; o.src_off = 0; o.src_cs = C; o.dst = dst; o.dst_off = dst_off; o.dst_cs = dst_cs; o.C = C; o.Hi = hi; o.Wi = wi;
        o.Ho = ho = kind == OP_MAXPOOL_S2 ? conv_out(hi, 3, 2, 0) : hi; o.Wo = wo = kind == OP_MAXPOOL_S2 ? conv_out(wi, 3, 2, 0) : wi;
        need(dst, o.Ho, o.Wo, dst_cs);
        p.ops.push_back(o);
    };
    auto side = [&] { p.sides.push_back({h, w}); };
    auto done = [&](int buf, int C) { p.out_buf = buf; p.out_C = C; p.out_H = h; p.out_W = w; p.ok = true; return p; };

    need(BUF_IN0, h, w, 3);
    conv("Conv2d_1a_3x3", BUF_IN0, 3, BUF_T0, 0, 32, h, w, h, w); side();
    conv("Conv2d_2a_3x3", BUF_T0, 32, BUF_T1, 0, 32, h, w, h, w); side();
    conv("Conv2d_2b_3x3", BUF_T1, 32, BUF_T0, 0, 64, h, w, h, w); side();
    pool(OP_MAXPOOL_S2, BUF_T0, 64, BUF_X, 0, 64, h, w, h, w); side();
    if (output_block == 0) return done(BUF_X, 64);
    conv("Conv2d_3b_1x1", BUF_X, 64, BUF_T0, 0, 80, h, w, h, w); side();
    conv("Conv2d_4a_3x3", BUF_T0, 80, BUF_T1, 0, 192, h, w, h, w); side();
    pool(OP_MAXPOOL_S2, BUF_T1, 192, BUF_Y, 0, 192, h, w, h, w); side();
    if (output_block == 1) return done(BUF_Y, 192);

    int cur = BUF_Y, nxt = BUF_X, cin = 192, t0, t1;      // t0 / t1: output sides of intermediates that keep the block's size
    auto begin = [&](const std::string& name, int width, int ho, int wo) { Block b; b.name = name; b.width = width; b.H = ho; b.W = wo; p.blocks.push_back(b); };
    auto slice = [&](const std::string& br, int off, int len) { p.blocks.back().slices.push_back({br, off, len}); };
    auto end = [&](int width) { std::swap(cur, nxt); cin = width; };

    const struct { const char* n; int pf; } A[3] = {{"Mixed_5b", 32}, {"Mixed_5c", 64}, {"Mixed_5d", 64}};
    for (const auto& a : A) {
        const std::string q = std::string(a.n) + ".";
        const int width = 64 + 64 + 96 + a.pf;
        begin(a.n, width, h, w);
        conv(q + "branch1x1", cur, cin, nxt, 0, width, h, w, t0, t1); slice("branch1x1", 0, 64);
        conv(q + "branch5x5_1", cur, cin, BUF_T0, 0, 48, h, w, t0, t1);
        conv(q + "branch5x5_2", BUF_T0, 48, nxt, 64, width, h, w, t0, t1); slice("branch5x5", 64, 64);
        conv(q + "branch3x3dbl_1", cur, cin, BUF_T0, 0, 64, h, w, t0, t1);
        conv(q + "branch3x3dbl_2", BUF_T0, 64, BUF_T1, 0, 96, h, w, t0, t1);
        conv(q + "branch3x3dbl_3", BUF_T1, 96, nxt, 128, width, h, w, t0, t1); slice("branch3x3dbl", 128, 96);
        pool(OP_AVGPOOL_S1, cur, cin, BUF_P, 0, cin, h, w, t0, t1);
        conv(q + "branch_pool", BUF_P, cin, nxt, 224, width, h, w, t0, t1); slice("branch_pool", 224, a.pf);
        end(width);
    }
    {
        const std::string q = "Mixed_6a.";
        const int ho = conv_out(h, 3, 2, 0), wo = conv_out(w, 3, 2, 0);
        begin("Mixed_6a", 768, ho, wo);
        conv(q + "branch3x3", cur, cin, nxt, 0, 768, h, w, t0, t1); slice("branch3x3", 0, 384);
        conv(q + "branch3x3dbl_1", cur, cin, BUF_T0, 0, 64, h, w, t0, t1);
        conv(q + "branch3x3dbl_2", BUF_T0, 64, BUF_T1, 0, 96, h, w, t0, t1);
        conv(q + "branch3x3dbl_3", BUF_T1, 96, nxt, 384, 768, h, w, t0, t1); slice("branch3x3dbl", 384, 96);
        pool(OP_MAXPOOL_S2, cur, cin, nxt, 480, 768, h, w, t0, t1); slice("maxpool", 480, 288);
        h = ho; w = wo; side();
        end(768);
    }
    const char* Cb[4] = {"Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"};
    for (const char* n : Cb) {
        const std::string q = std::string(n) + ".";
        const int c7 = layers()[layer_index(q + "branch7x7_1")].Cout;
        begin(n, 768, h, w);
        conv(q + "branch1x1", cur, cin, nxt, 0, 768, h, w, t0, t1); slice("branch1x1", 0, 192);
        conv(q + "branch7x7_1", cur, cin, BUF_T0, 0, c7, h, w, t0, t1);
        conv(q + "branch7x7_2", BUF_T0, c7, BUF_T1, 0, c7, h, w, t0, t1);
        conv(q + "branch7x7_3", BUF_T1, c7, nxt, 192, 768, h, w, t0, t1); slice("branch7x7", 192, 192);
        conv(q + "branch7x7dbl_1", cur, cin, BUF_T0, 0, c7, h, w, t0, t1);
        conv(q + "branch7x7dbl_2", BUF_T0, c7, BUF_T1, 0, c7, h, w, t0, t1);
        conv(q + "branch7x7dbl_3", BUF_T1, c7, BUF_T0, 0, c7, h, w, t0, t1);
        conv(q + "branch7x7dbl_4", BUF_T0, c7, BUF_T1, 0, c7, h, w, t0, t1);
        conv(q + "branch7x7dbl_5", BUF_T1, c7, nxt, 384, 768, h, w, t0, t1); slice("branch7x7dbl", 384, 192);
        pool(OP_AVGPOOL_S1, cur, cin, BUF_P, 0, cin, h, w, t0, t1);
        conv(q + "branch_pool", BUF_P, cin, nxt, 576, 768, h, w, t0, t1); slice("branch_pool", 576, 192);
        end(768);
    }
    if (output_block == 2) return done(cur, 768);
    {
        const std::string q = "Mixed_7a.";
        const int ho = conv_out(h, 3, 2, 0), wo = conv_out(w, 3, 2, 0);
        if (ho < 1 || wo < 1) { p.err = "Inception: no pixel left for Mixed_7a"; return p; }      // unreachable past the side rule above; kept as the guard of the launches
        begin("Mixed_7a", 1280, ho, wo);
        conv(q + "branch3x3_1", cur, cin, BUF_T0, 0, 192, h, w, t0, t1);
        conv(q + "branch3x3_2", BUF_T0, 192, nxt, 0, 1280, h, w, t0, t1); slice("branch3x3", 0, 320);
        conv(q + "branch7x7x3_1", cur, cin, BUF_T0, 0, 192, h, w, t0, t1);
        conv(q + "branch7x7x3_2", BUF_T0, 192, BUF_T1, 0, 192, h, w, t0, t1);
        conv(q + "branch7x7x3_3", BUF_T1, 192, BUF_T0, 0, 192, h, w, t0, t1);
        conv(q + "branch7x7x3_4", BUF_T0, 192, nxt, 320, 1280, h, w, t0, t1); slice("branch7x7x3", 320, 192);
        pool(OP_MAXPOOL_S2, cur, cin, nxt, 512, 1280, h, w, t0, t1); slice("maxpool", 512, 768);
        h = ho; w = wo; side();
        end(1280);
    }
    const char* E[2] = {"Mixed_7b", "Mixed_7c"};
    for (int e = 0; e < 2; ++e) {
        const std::string q = std::string(E[e]) + ".";
        begin(E[e], 2048, h, w);
        conv(q + "branch1x1", cur, cin, nxt, 0, 2048, h, w, t0, t1); slice("branch1x1", 0, 320);
        conv(q + "branch3x3_1", cur, cin, BUF_T0, 0, 384, h, w, t0, t1);
        conv(q + "branch3x3_2a", BUF_T0, 384, nxt, 320, 2048, h, w, t0, t1); slice("branch3x3_2a", 320, 384);
        conv(q + "branch3x3_2b", BUF_T0, 384, nxt, 704, 2048, h, w, t0, t1); slice("branch3x3_2b", 704, 384);
        conv(q + "branch3x3dbl_1", cur, cin, BUF_T0, 0, 448, h, w, t0, t1);
        conv(q + "branch3x3dbl_2", BUF_T0, 448, BUF_T1, 0, 384, h, w, t0, t1);
        conv(q + "branch3x3dbl_3a", BUF_T1, 384, nxt, 1088, 2048, h, w, t0, t1); slice("branch3x3dbl_3a", 1088, 384);
        conv(q + "branch3x3dbl_3b", BUF_T1, 384, nxt, 1472, 2048, h, w, t0, t1); slice("branch3x3dbl_3b", 1472, 384);
        pool(e == 0 ? OP_AVGPOOL_S1 : OP_MAXPOOL_S1, cur, cin, BUF_P, 0, cin, h, w, t0, t1);      // 7c's max pool is the FID network's own (models.py:812-816)
        conv(q + "branch_pool", BUF_P, cin, nxt, 1856, 2048, h, w, t0, t1); slice("branch_pool", 1856, 192);
        end(2048);
    }
    return done(cur, 2048);
}

}  // namespace inc
}  // namespace pf
