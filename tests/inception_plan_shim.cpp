// extern "C" wrappers around pnpflow_amd/csrc/inception_plan.h for tests/test_inception_host.py (plain host C++17, no HIP).  Compiled with
// -DINC_PLAN_MAIN it is a stand-alone program that walks the planner over a set of inputs (the build the sanitizers run on).
#include <cstdio>
#include <cstring>

#include "inception_plan.h"

using namespace pf::inc;

extern "C" {

int ip_num_layers() { return (int)layers().size(); }
// dims: Cin, Cout, KH, KW, S, PH, PW
int ip_layer(int i, char* name, int cap, int* dims) {
    if (i < 0 || i >= (int)layers().size() || cap < 1) return -1;
    const Layer& l = layers()[i];
    std::snprintf(name, (size_t)cap, "%s", l.name.c_str());
    const int v[7] = {l.Cin, l.Cout, l.KH, l.KW, l.S, l.PH, l.PW};
    std::memcpy(dims, v, sizeof(v));
    return 0;
}
int ip_choose_tile(long long M, int Cout) { return choose_tile(M, Cout); }
int ip_tile_mt(int t) { return tile_mt(t); }
int ip_tile_nt(int t) { return tile_nt(t); }

// head: ok, number of ops, number of blocks, number of sides, out_buf, out_C, out_H, out_W, H0, W0; err: the refusal text
int ip_plan(int B, int H, int W, int resize, int output_block, long long* head, long long* buf_floats, char* err, int err_cap) {
    const Plan p = plan(B, H, W, resize != 0, output_block);
    const long long v[10] = {p.ok, (long long)p.ops.size(), (long long)p.blocks.size(), (long long)p.sides.size(), p.out_buf, p.out_C, p.out_H, p.out_W, p.H0, p.W0};
    std::memcpy(head, v, sizeof(v));
    for (int b = 0; b < NUM_BUFS; ++b) buf_floats[b] = (long long)p.buf_floats[b];
    std::snprintf(err, (size_t)err_cap, "%s", p.err.c_str());
    return p.ok ? 0 : -1;
}
// 14 values: kind, layer, src, src_off, src_cs, dst, dst_off, dst_cs, C, Hi, Wi, Ho, Wo, tile
int ip_op(int B, int H, int W, int resize, int output_block, int i, int* out) {
    const Plan p = plan(B, H, W, resize != 0, output_block);
    if (!p.ok || i < 0 || i >= (int)p.ops.size()) return -1;
    const Op& o = p.ops[i];
    const int v[14] = {o.kind, o.layer, o.src, o.src_off, o.src_cs, o.dst, o.dst_off, o.dst_cs, o.C, o.Hi, o.Wi, o.Ho, o.Wo, o.tile};
    std::memcpy(out, v, sizeof(v));
    return 0;
}
// block i: name, (width, H, W, number of slices), then up to 8 (off, len) pairs
int ip_block(int B, int H, int W, int resize, int output_block, int i, char* name, int cap, int* head, int* slices) {
    const Plan p = plan(B, H, W, resize != 0, output_block);
    if (!p.ok || i < 0 || i >= (int)p.blocks.size()) return -1;
    const Block& b = p.blocks[i];
    std::snprintf(name, (size_t)cap, "%s", b.name.c_str());
    head[0] = b.width; head[1] = b.H; head[2] = b.W; head[3] = (int)b.slices.size();
    for (size_t k = 0; k < b.slices.size() && k < 8; ++k) { slices[2 * k] = b.slices[k].off; slices[2 * k + 1] = b.slices[k].len; }
    return 0;
}
int ip_side(int B, int H, int W, int resize, int output_block, int i, int* hw) {
    const Plan p = plan(B, H, W, resize != 0, output_block);
    if (!p.ok || i < 0 || i >= (int)p.sides.size()) return -1;
    hw[0] = p.sides[i].first; hw[1] = p.sides[i].second;
    return 0;
}

}  // extern "C"

#ifdef INC_PLAN_MAIN
// every plan a test or a user can ask for in one sweep: the checks are bounds of the plan's own tables (every slice inside its tensor, every
// tensor inside its buffer); the sanitizers watch the planner's memory while it runs
int main() {
    long long plans = 0, refused = 0;
    for (int side : {1, 64, 74, 75, 76, 139, 299, 300, 512})
        for (int resize = 0; resize < 2; ++resize)
            for (int blk = -1; blk <= 4; ++blk)
                for (int B : {0, 1, 2, 50}) {
                    const Plan p = plan(B, side, side == 139 ? 151 : side, resize != 0, blk);
                    ++plans;
                    if (!p.ok) { ++refused; if (p.err.empty()) { std::printf("refusal without a message\n"); return 1; } continue; }
                    for (const Op& o : p.ops) {
                        const bool conv = o.kind == OP_CONV;
                        const int width = conv ? layers()[o.layer].Cout : o.C;
                        if (o.dst_off < 0 || o.dst_off + width > o.dst_cs || o.src_off + o.C > o.src_cs) { std::printf("slice outside its tensor\n"); return 1; }
                        if ((size_t)B * o.Ho * o.Wo * o.dst_cs > p.buf_floats[o.dst] || (size_t)B * o.Hi * o.Wi * o.src_cs > p.buf_floats[o.src]) {
                            std::printf("tensor outside its buffer\n"); return 1;
                        }
                        if (conv && (o.tile < 0 || o.tile >= NUM_TILES)) { std::printf("conv without a tile\n"); return 1; }
                    }
                }
    std::printf("inception_plan: %lld plans, %lld refused, %d layers: ok\n", plans, refused, (int)layers().size());
    return 0;
}
#endif
