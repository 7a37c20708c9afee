// CPU check of the weight-gradient overlap schedule (voicebox-pytorch_amd/csrc/wgrad_overlap_plan.hpp, executed by runtime.hip).
//
// For a backward of L layers the plan header emits every launch with the resources it reads and writes, and every event record /
// wait, in submission order.  This program builds the happens-before relation from them -- order within the caller's stream, order
// within the side stream, record -> wait -- and asserts, for every pair of accesses to one resource of which at least one writes,
// that the one submitted first happens before the other.  That covers, for the operands of wgrad(l) and reduce(l) (buffer copies,
// side slab regions, the layer's gradient ranges + sq_partials):
//   * written before read            (the chain's writer -> FORK -> the grouped launch; the launch -> the reduce)
//   * not overwritten until read     (the grouped launch -> GEMM event -> the chain's next writer of that copy, two layers on)
//   * final before the caller's next operation (every reduce -> JOIN -> whatever follows the embed stage: modelled as one launch
//     on the caller's stream that reads and writes everything)
// Two scenarios: one whole backward; and a backward abandoned after its first layer followed by a whole one (the head's wait).
// Self-check: with any single wait of the whole backward removed, at least one scenario must report a violation -- so every wait
// of the plan is necessary and the checker can see each of them.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../voicebox-pytorch_amd/csrc/wgrad_overlap_plan.hpp"

using namespace wgrad_overlap;

struct Item {
  Op op;
  int wait_id;  // ordinal of this wait inside the final (whole) backward, -1 otherwise
};

static std::string res_name(const Res& r) {
  static const char* bufs[] = {"dxb", "dh1", "dxb2", "dqkv"};
  char t[64];
  switch (r.kind) {
    case RES_BUF: snprintf(t, sizeof t, "%s[%d]", bufs[r.a], r.b); break;
    case RES_SLABS_MAIN: snprintf(t, sizeof t, "slabs(main)"); break;
    case RES_SLABS_SIDE: snprintf(t, sizeof t, "slabs(side)"); break;
    case RES_WGRAD: snprintf(t, sizeof t, "grads+sq(layer %d)", r.a); break;
    case RES_GRAD_HEAD: snprintf(t, sizeof t, "grads(head)"); break;
    case RES_GRAD_EMBED: snprintf(t, sizeof t, "grads(embed)"); break;
    case RES_FWD_ACTS: snprintf(t, sizeof t, "forward activations"); break;
  }
  return t;
}

// the caller's next operation: the optimizer reads every gradient, the next forward and backward rewrite every buffer
static Op next_operation(int L) {
  Op o{};
  o.type = Op::LAUNCH; o.stream = MAIN; o.name = "next operation"; o.layer = -1;
  return o;  // its resource list is "everything": handled in check()
}

static std::vector<Item> build(int L, bool abandoned_first) {
  std::vector<Item> ops;
  int waits = 0;
  bool final_pass = false;
  auto sink = [&](const Op& o) {
    Item it{o, -1};
    if (final_pass && o.type == Op::SYNC && o.sync.kind == SYNC_WAIT) it.wait_id = waits++;
    ops.push_back(it);
  };
  if (abandoned_first) {
    emit_head(L, sink);
    emit_layer(L - 1, L, sink);
  }
  final_pass = true;
  emit_backward(L, sink);
  ops.push_back({next_operation(L), -1});
  return ops;
}

struct Access {
  int stream, idx, item;
  bool write;
};

// returns the number of violations; verbose: print them.  skip_wait: ordinal of the wait to leave out (-1: none)
static int check(int L, const std::vector<Item>& ops, int skip_wait, bool verbose, bool need_writer) {
  int count[2] = {0, 0};
  int cur[2][2] = {{0, 0}, {0, 0}};  // cur[s][t]: the latest op of stream t that stream s is ordered after (1-based, 0 none)
  int evclock[EV_N][2] = {};
  bool recorded[EV_N] = {};
  std::map<std::tuple<int, int, int>, std::vector<Access>> acc;
  int bad = 0;
  auto touch = [&](const Item& it, int item, const Res& r, bool write, int s, int idx, const int clock[2]) {
    auto& v = acc[std::make_tuple((int)r.kind, r.a, r.b)];
    bool writer_seen = false;
    for (const Access& p : v) {
      writer_seen |= p.write;
      if (!p.write && !write) continue;
      if (clock[p.stream] >= p.idx) continue;  // p happens before this access
      bad++;
      if (verbose)
        printf("  L=%d VIOLATION on %s: '%s' (layer %d) %s it while '%s' (layer %d) may still %s it\n", L, res_name(r).c_str(), it.op.name,
               it.op.layer, write ? "writes" : "reads", ops[p.item].op.name, ops[p.item].op.layer, p.write ? "write" : "read");
    }
    if (!write && need_writer && it.op.stream == SIDE && !writer_seen) {
      bad++;
      if (verbose) printf("  L=%d VIOLATION on %s: '%s' (layer %d) reads it and nothing wrote it\n", L, res_name(r).c_str(), it.op.name, it.op.layer);
    }
    v.push_back({s, idx, item, write});
  };
  for (int i = 0; i < (int)ops.size(); i++) {
    const Item& it = ops[i];
    const int s = it.op.stream;
    const int idx = ++count[s];
    cur[s][s] = idx;
    if (it.op.type == Op::SYNC) {
      const Sync& y = it.op.sync;
      if (y.kind == SYNC_RECORD) {
        evclock[y.ev][0] = cur[s][0]; evclock[y.ev][1] = cur[s][1];
        recorded[y.ev] = true;
      } else if (y.kind == SYNC_WAIT && !(it.wait_id >= 0 && it.wait_id == skip_wait) && recorded[y.ev]) {
        for (int t = 0; t < 2; t++) if (evclock[y.ev][t] > cur[s][t]) cur[s][t] = evclock[y.ev][t];
      }
      continue;
    }
    if (!strcmp(it.op.name, "next operation")) {  // reads and writes every resource seen so far
      std::vector<std::tuple<int, int, int>> keys;
      for (auto& kv : acc) keys.push_back(kv.first);
      for (auto& k : keys) touch(it, i, Res{(ResKind)std::get<0>(k), std::get<1>(k), std::get<2>(k)}, true, s, idx, cur[s]);
      continue;
    }
    for (int r = 0; r < it.op.nr; r++) touch(it, i, it.op.reads[r], false, s, idx, cur[s]);
    for (int w = 0; w < it.op.nw; w++) touch(it, i, it.op.writes[w], true, s, idx, cur[s]);
  }
  return bad;
}

int main() {
  const int Ls[] = {1, 2, 3, 4, 5, 12, 24};
  int failures = 0;
  for (int L : Ls) {
    const std::vector<Item> whole = build(L, false), after_abandoned = build(L, true);
    int nwaits = 0;
    for (const Item& it : whole) if (it.wait_id >= 0) nwaits++;
    // the forward activations are written by the forward, outside this model: only the side stream's other operands need a writer
    int bad = check(L, whole, -1, true, false) + check(L, after_abandoned, -1, true, false);
    {  // every buffer copy and slab region a side-stream launch reads was written earlier in this backward
      std::vector<Item> w2;
      for (Item it : whole) {
        if (it.op.type == Op::LAUNCH) {  // drop the forward activations from the read lists for this pass
          int k = 0;
          for (int r = 0; r < it.op.nr; r++) if (it.op.reads[r].kind != RES_FWD_ACTS) it.op.reads[k++] = it.op.reads[r];
          it.op.nr = k;
        }
        w2.push_back(it);
      }
      bad += check(L, w2, -1, true, true);
    }
    // the copies are distinct where the plan needs them to be: a layer never reads and writes the same dxb copy
    for (int l = 0; l < L; l++)
      if (dxb_read_copy(l) == write_copy(BUF_DXB, l)) { printf("  L=%d layer %d reads and writes dxb[%d]\n", L, l, dxb_read_copy(l)); bad++; }
    int blind = 0;
    for (int k = 0; k < nwaits; k++) {
      const int v = check(L, whole, k, false, false) + check(L, after_abandoned, k, false, false);
      if (v == 0) {
        blind++;
        printf("  L=%d SELF-CHECK: removing wait #%d of the backward goes unnoticed\n", L, k);
      }
    }
    printf("L=%2d: %3d launches and syncs, %2d waits, %d violations, %d waits whose removal goes unnoticed\n", L, (int)whole.size(), nwaits,
           bad, blind);
    failures += bad + blind;
  }
  if (failures) { printf("FAILED\n"); return 1; }
  printf("wgrad overlap plan ok\n");
  return 0;
}
