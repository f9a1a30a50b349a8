#include "dc_record.h"
#include <algorithm>
#include <cstring>

namespace dc {

using rec::kMaxLayers;
using rec::kMetaStride;

bool HostRecord::build(const dc_record &r, int B, int N, int cap, int np, const std::vector<int> &user_of, const std::vector<int> &dev_of) {
  auto refuse = [&](int c, const std::string &msg) { code = c; error = msg; return false; };
  auto dev = [&](int u) { return dev_of.empty() ? u : dev_of[u]; };
  code = DC_OK; error.clear();
  prim.assign((size_t) B * N, -1);
  for (int b = 0; b < B; b++)
    for (int i = 0; i < N; i++) {
      const int q = r.prim[(size_t) b * N + (user_of.empty() ? i : user_of[i])];
      if (q >= np) return refuse(DC_ERR_INVALID, "dc_set_record: primitive index out of range");
      prim[(size_t) b * N + i] = q < 0 ? -1 : q;
    }
  meta.assign((size_t) B * kMetaStride, 0); verts.assign((size_t) B * 2 * cap, 0);
  pair.assign((size_t) B * cap, rec::Int2{0, 0});
  nrm.assign((size_t) B * cap, rec::Float4{0, 0, 0, 0}); dvec.assign((size_t) B * cap, rec::Float4{0, 0, 0, 0});
  sn.assign((size_t) B * cap * 3, 0.0); sd.assign((size_t) B * cap * 3, 0.0);
  size_t at = 0;      // the lists of the rollouts are concatenated
  for (int b = 0; b < B && r.self_count; b++) {
    const int C = r.self_count[b];
    if (C < 0 || C > cap) return refuse(DC_ERR_CAPACITY, "dc_set_record: more self contacts than max_self_contacts = " + std::to_string(cap));
    int *m = meta.data() + (size_t) b * kMetaStride;
    std::vector<int> ids, in_layer((size_t) N, -1);      // (in_layer: the last layer a vertex appeared in)
    int nl = 0;
    for (int k = 0; k < C; k++) {
      const int p1 = r.self_pairs[2 * (at + k)], p2 = r.self_pairs[2 * (at + k) + 1], l = r.self_layer[at + k];
      if (p1 < 0 || p2 >= N || p1 >= p2) return refuse(DC_ERR_INVALID, "dc_set_record: self contact pair must satisfy 0 <= id1 < id2 < N");
      if (l < 0 || l >= kMaxLayers || (k > 0 && l < r.self_layer[at + k - 1])) return refuse(DC_ERR_INVALID, "dc_set_record: self contacts must come in layer order");
      // the contacts of a layer are applied in parallel (Simulation::contactSorting, Simulation.cpp:422-624, builds them vertex-disjoint)
      if (in_layer[p1] == l || in_layer[p2] == l) return refuse(DC_ERR_INVALID, "dc_set_record: rollout " + std::to_string(b) + ": a vertex appears twice in self-contact layer " + std::to_string(l));
      in_layer[p1] = in_layer[p2] = l;
      nl = std::max(nl, l + 1);
      ids.push_back(p1); ids.push_back(p2);
    }
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const int M = (int) ids.size();
    m[0] = C; m[1] = C > 0 ? nl : 0;
    for (int k = 0; k < C; k++) m[2 + r.self_layer[at + k] + 1]++;
    for (int l = 0; l < nl; l++) m[2 + l + 1] += m[2 + l];
    m[kMetaStride - 1] = M; m[kMetaStride - 2] = 0; m[kMetaStride - 3] = C;
    for (int q = 0; q < M; q++) verts[(size_t) b * 2 * cap + q] = dev(ids[q]);
    for (int k = 0; k < C; k++) {
      const int p1 = r.self_pairs[2 * (at + k)], p2 = r.self_pairs[2 * (at + k) + 1];
      const int s1 = (int) (std::lower_bound(ids.begin(), ids.end(), p1) - ids.begin()), s2 = (int) (std::lower_bound(ids.begin(), ids.end(), p2) - ids.begin());
      const size_t o = (size_t) b * cap + k;
      const double *n = r.self_normal + 3 * (at + k), *d = r.self_d + 3 * (at + k);
      pair[o] = rec::Int2{dev(p1), dev(p2)};
      const int slots = s1 | (s2 << 16);
      float w; std::memcpy(&w, &slots, sizeof(float));
      nrm[o] = rec::Float4{(float) n[0], (float) n[1], (float) n[2], w};
      dvec[o] = rec::Float4{(float) d[0], (float) d[1], (float) d[2], 0.f};
      for (int q = 0; q < 3; q++) { sn[3 * o + q] = n[q]; sd[3 * o + q] = d[q]; }
    }
    at += C;
  }
  return true;
}

}  // namespace dc
