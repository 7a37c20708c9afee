// The schedule of the backward's weight-gradient overlap, as data.  Host-only C++ (no HIP): runtime.hip executes it, and
// tests/native/wgrad_overlap_plan_check.cpp builds the happens-before graph of a whole backward from it and checks every operand.
//
// A layer's backward is a serial chain of launches on the caller's stream (MAIN) that carries dx from layer L-1 down to layer 0.
// The layer's four weight-gradient GEMMs (one grouped launch) and their slab reduce read what the chain left behind and nothing in
// the chain reads their results, so they run on a second stream (SIDE) beside the next layer's chain.  Three things keep that exact:
//   copies   every scratch buffer that wgrad(l) reads and the chain would overwrite before SIDE is done exists in 2 (dxb: 3) copies,
//            indexed by layer, so that the first overwrite of a copy is two layers after its reader was submitted;
//   events   FORK (MAIN, after dgrad to_qkv: every operand of wgrad(l) is written), GEMM0 / GEMM1 (SIDE, after the grouped launch of
//            an even / odd layer: its operands are free), JOIN (SIDE, after every slab reduce);
//   waits    SIDE waits for FORK before the grouped launch; MAIN waits at the start of layer l for the GEMM event of layer l + 2,
//            the last reader of every copy that layer l writes; MAIN waits for JOIN at the end of the embed stage (the last call of a
//            backward: gradients and sq_partials are final for whatever the caller runs next) and at the start of the head stage
//            (a backward that was abandoned half way leaves nothing in flight under the next one).
// SIDE has its own four slab regions; it is one in-order stream, so wgrad(l - 1) overwrites them after reduce(l) has read them.
#pragma once
#include <initializer_list>

namespace wgrad_overlap {

// ---- buffer copies
enum Buf { BUF_DXB, BUF_DH1, BUF_DXB2, BUF_DQKV, BUF_N };
constexpr int kMaxCopies = 3;
constexpr int copies(Buf b) { return b == BUF_DXB ? 3 : 2; }
// the copy of `b` that layer l writes.  dxb is written by the layer's LAST launch (the norm backward that hands bf16 dx to layer
// l - 1) and read by the layer below and by its wgrad; the others are written and read inside layer l.  Layer 0 writes copy 0.
constexpr int write_copy(Buf b, int l) { return l % copies(b); }
// the dxb copy that layer l reads: what layer l + 1 wrote (for l = L - 1: what the head stage writes)
constexpr int dxb_read_copy(int l) { return write_copy(BUF_DXB, l + 1); }

// ---- events and sync points
enum Stream { MAIN, SIDE };
enum Event { EV_FORK, EV_GEMM0, EV_GEMM1, EV_JOIN, EV_N };
constexpr Event gemm_event(int l) { return (l & 1) ? EV_GEMM1 : EV_GEMM0; }
// the layer whose grouped launch must be over before layer l overwrites the copies it writes (-1: none)
constexpr int last_reader(int l, int L) { return l + 2 < L ? l + 2 : -1; }

enum Point {
  PT_HEAD_BEGIN,         // vbx_model_backward_head, before its first launch
  PT_LAYER_BEGIN,        // vbx_model_backward_layer, before its first launch
  PT_FORK,               // MAIN, after dgrad to_qkv
  PT_SIDE_BEGIN,         // SIDE, before the grouped wgrad launch
  PT_SIDE_GEMM_DONE,     // SIDE, after the grouped wgrad launch
  PT_SIDE_REDUCE_DONE,   // SIDE, after the slab reduce
  PT_EMBED_END,          // vbx_model_backward_embed, after its last launch
};
enum SyncKind { SYNC_NONE, SYNC_RECORD, SYNC_WAIT };
struct Sync {
  SyncKind kind;
  Stream stream;  // the stream that records / waits
  Event ev;
};
// what happens at point p of layer l (l is ignored at the head / embed points) in a backward of L layers
constexpr Sync sync_at(Point p, int l, int L) {
  switch (p) {
    case PT_HEAD_BEGIN: return {SYNC_WAIT, MAIN, EV_JOIN};
    case PT_LAYER_BEGIN: return last_reader(l, L) >= 0 ? Sync{SYNC_WAIT, MAIN, gemm_event(last_reader(l, L))} : Sync{SYNC_NONE, MAIN, EV_N};
    case PT_FORK: return {SYNC_RECORD, MAIN, EV_FORK};
    case PT_SIDE_BEGIN: return {SYNC_WAIT, SIDE, EV_FORK};
    case PT_SIDE_GEMM_DONE: return {SYNC_RECORD, SIDE, gemm_event(l)};
    case PT_SIDE_REDUCE_DONE: return {SYNC_RECORD, SIDE, EV_JOIN};
    case PT_EMBED_END: return {SYNC_WAIT, MAIN, EV_JOIN};
  }
  return {SYNC_NONE, MAIN, EV_N};
}

// ---- the launches of a backward and what they touch, in submission order (the checker's model of runtime.hip; the runtime itself
// takes the copies and the sync points from the functions above).  Resources: a buffer copy, a slab set, the weight-gradient
// ranges + sq_partials of a layer, the gradients of the head / embed stages, the saved forward activations.
enum ResKind { RES_BUF, RES_SLABS_MAIN, RES_SLABS_SIDE, RES_WGRAD, RES_GRAD_HEAD, RES_GRAD_EMBED, RES_FWD_ACTS };
struct Res {
  ResKind kind;
  int a, b;  // RES_BUF: Buf, copy; RES_WGRAD: layer
};
struct Op {
  enum Type { LAUNCH, SYNC } type;
  Stream stream;
  const char* name;
  int layer;  // -1: head / embed
  Sync sync;          // SYNC
  Point point;        // SYNC
  Res reads[6], writes[4];
  int nr, nw;
};

template <class F>
inline void emit_sync(Point p, int l, int L, F&& f) {
  const Sync s = sync_at(p, l, L);
  if (s.kind == SYNC_NONE) return;
  Op o{};
  o.type = Op::SYNC; o.stream = s.stream; o.name = s.kind == SYNC_WAIT ? "wait" : "record"; o.layer = l; o.sync = s; o.point = p;
  f(o);
}
template <class F>
inline void emit_launch(Stream st, const char* name, int l, std::initializer_list<Res> reads, std::initializer_list<Res> writes, F&& f) {
  Op o{};
  o.type = Op::LAUNCH; o.stream = st; o.name = name; o.layer = l;
  for (const Res& r : reads) o.reads[o.nr++] = r;
  for (const Res& w : writes) o.writes[o.nw++] = w;
  f(o);
}

template <class F>
inline void emit_head(int L, F&& f) {
  emit_sync(PT_HEAD_BEGIN, -1, L, f);
  emit_launch(MAIN, "to_pred wgrad + reduce", -1, {{RES_FWD_ACTS, 0, 0}}, {{RES_SLABS_MAIN, 0, 0}, {RES_GRAD_HEAD, 0, 0}}, f);
  emit_launch(MAIN, "final norm backward", -1, {{RES_FWD_ACTS, 0, 0}}, {{RES_BUF, BUF_DXB, dxb_read_copy(L - 1)}}, f);
}
template <class F>
inline void emit_layer(int l, int L, F&& f) {
  const Res dxb_in{RES_BUF, BUF_DXB, dxb_read_copy(l)}, dxb_out{RES_BUF, BUF_DXB, write_copy(BUF_DXB, l)};
  const Res dh1{RES_BUF, BUF_DH1, write_copy(BUF_DH1, l)}, dxb2{RES_BUF, BUF_DXB2, write_copy(BUF_DXB2, l)};
  const Res dqkv{RES_BUF, BUF_DQKV, write_copy(BUF_DQKV, l)}, acts{RES_FWD_ACTS, 0, 0};
  emit_sync(PT_LAYER_BEGIN, l, L, f);
  emit_launch(MAIN, "dgrad ff_out", l, {dxb_in}, {}, f);
  emit_launch(MAIN, "GEGLU backward", l, {acts}, {dh1}, f);
  emit_launch(MAIN, "dgrad ff_in", l, {dh1}, {}, f);
  emit_launch(MAIN, "norm backward (ff)", l, {acts}, {dxb2}, f);
  emit_launch(MAIN, "dgrad to_out", l, {dxb2}, {}, f);
  emit_launch(MAIN, "attention backward", l, {acts}, {dqkv}, f);
  emit_launch(MAIN, "dgrad to_qkv", l, {dqkv}, {}, f);
  emit_sync(PT_FORK, l, L, f);
  emit_sync(PT_SIDE_BEGIN, l, L, f);
  emit_launch(SIDE, "wgrad (4 GEMMs)", l, {dxb_in, dh1, dxb2, dqkv, acts}, {{RES_SLABS_SIDE, 0, 0}}, f);
  emit_sync(PT_SIDE_GEMM_DONE, l, L, f);
  emit_launch(SIDE, "wgrad slab reduce", l, {{RES_SLABS_SIDE, 0, 0}}, {{RES_WGRAD, l, 0}}, f);
  emit_sync(PT_SIDE_REDUCE_DONE, l, L, f);
  emit_launch(MAIN, "norm backward (attn)", l, {acts}, {dxb_out}, f);
}
template <class F>
inline void emit_embed(int L, F&& f) {
  emit_launch(MAIN, "to_embed wgrad + reduce", -1, {{RES_FWD_ACTS, 0, 0}}, {{RES_SLABS_MAIN, 0, 0}, {RES_GRAD_EMBED, 0, 0}}, f);
  emit_sync(PT_EMBED_END, -1, L, f);
}
// head, layers L-1 .. 0, embed
template <class F>
inline void emit_backward(int L, F&& f) {
  emit_head(L, f);
  for (int l = L - 1; l >= 0; l--) emit_layer(l, L, f);
  emit_embed(L, f);
}

}  // namespace wgrad_overlap
