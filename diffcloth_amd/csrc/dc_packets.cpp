#include "dc_packets.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace dc {

bool HostPackets::build(const HostSystem &H, int want_threads) {
  const int shape = pk_shape_for(H.N, want_threads);      // (dc_kernelplan.h: the instances of k_pd_step_pk)
  if (shape < 0) {          // too large for the one-workgroup kernel: report the bandwidth, no tables
    *this = HostPackets();
    for (int r = 0; r < H.N; r++)
      for (int k = H.P_ptr[r]; k < H.P_ptr[r + 1]; k++) bandwidth = std::max(bandwidth, std::abs(H.P_col[k] - r));
    return false;
  }
  const PkShape &s = kPkShapes[shape];
  if (!build_rows(H, s.threads * s.vpt)) return false;
  vpt = s.vpt; threads = s.threads; this->shape = shape;
  return true;
}

bool HostPackets::build_rows(const HostSystem &H, int rows_padded) {
  *this = HostPackets();
  const int N = H.N;
  for (int r = 0; r < N; r++)
    for (int k = H.P_ptr[r]; k < H.P_ptr[r + 1]; k++) bandwidth = std::max(bandwidth, std::abs(H.P_col[k] - r));
  if (bandwidth > 511 || rows_padded < N || rows_padded % 64 != 0) return false;
  const int NPk = rows_padded, nch = NPk / 64, PBk = 4;
  std::vector<double> sq(N);
  sq_dinv.assign(NPk, 0.f);
  for (int i = 0; i < N; i++) {
    double d = 0;
    for (int k = H.P_ptr[i]; k < H.P_ptr[i + 1]; k++) if (H.P_col[k] == i) d = H.P_val[k];
    const float dinv = (float) (1.0 / d);              // the fp32 preconditioner entry the other kernels use
    sq[i] = std::sqrt((double) dinv);
    sq_dinv[i] = (float) sq[i];
  }
  pk_ptr.assign(nch, 0); pk_n.assign(nch, 0);
  for (int ch = 0; ch < nch; ch++) {
    int w = 0;
    for (int r = 64 * ch; r < std::min(N, 64 * ch + 64); r++) w = std::max(w, H.P_ptr[r + 1] - H.P_ptr[r] - 1);
    const int np = std::max(PBk, ((w + 2) / 3 + PBk - 1) / PBk * PBk);
    pk_ptr[ch] = (int) (pk.size() / 4); pk_n[ch] = np;
    pk.resize(pk.size() + (size_t) 4 * 64 * np, 0);
    for (int l = 0; l < 64; l++) {
      const int r = 64 * ch + l;
      int kk = r < N ? H.P_ptr[r] : 0;
      const int kend = r < N ? H.P_ptr[r + 1] : 0;
      for (int s = 0; s < np; s++) {
        int bits[3] = {0, 0, 0}, wd = 0;
        for (int q = 0; q < 3; q++) {
          int d = 512;
          while (kk < kend && H.P_col[kk] == r) kk++;          // the diagonal is implicit (= 1 after scaling)
          if (kk < kend) {
            const int col = H.P_col[kk];
            const float v = (float) (H.P_val[kk] * sq[r] * sq[col]);
            std::memcpy(&bits[q], &v, sizeof(int));
            d = col - r + 512;
            kk++;
          }
          wd |= d << (10 * q);
        }
        const size_t o = 4 * ((size_t) pk_ptr[ch] + (size_t) s * 64 + l);
        pk[o] = bits[0]; pk[o + 1] = bits[1]; pk[o + 2] = bits[2]; pk[o + 3] = wd;
      }
    }
  }
  ok = true;
  return true;
}

void HostPackets::to_offsets() {
  if (!ok || ofs) return;
  std::vector<int> out, ptr(pk_ptr.size(), 0);
  for (size_t ch = 0; ch < pk_ptr.size(); ch++) {
    const int nb = pk_n[ch] / 4;
    ptr[ch] = (int) (out.size() / 4);
    out.resize(out.size() + (size_t) 4 * kPkOfsBatchInt4 * nb, 0);
    for (int t = 0; t < nb; t++) {
      int *b = &out[4 * ((size_t) ptr[ch] + (size_t) kPkOfsBatchInt4 * t)];
      for (int l = 0; l < 64; l++) {
        unsigned o[12];
        for (int j = 0; j < 4; j++) {
          const int *q = &pk[4 * ((size_t) pk_ptr[ch] + (size_t) (4 * t + j) * 64 + l)];
          for (int k = 0; k < 3; k++) {
            const int n = 3 * j + k;                                 // non-zero n of the batch: value dword n, offset field n
            b[4 * (32 + 64 * (n / 4) + l) + n % 4] = q[k];
            o[n] = 8u * (((unsigned) q[3] >> (10 * k)) & 1023u);
          }
        }
        for (int w = 0; w < 4; w++) b[4 * (32 + 64 * 3 + l) + w] = (int) (o[2 * w] | o[2 * w + 1] << 16);
        for (int w = 0; w < 2; w++) b[2 * l + w] = (int) (o[8 + 2 * w] | o[9 + 2 * w] << 16);
      }
    }
  }
  pk.swap(out); pk_ptr.swap(ptr);
  ofs = true;
}

bool HostPackets::to_template() {
  if (!ok || !ofs || tpl) return false;
  const size_t nch = pk_ptr.size();
  for (size_t ch = 0; ch < nch; ch++) if (pk_n[ch] != 4) return false;      // a row of more than one batch
  // entry n of row (ch, l): value bits and column - row; the padding entries sit on the row itself (offset 0, value 0)
  auto entry = [&](size_t ch, int l, int n, int &bits) {
    const int *b = &pk[4 * (size_t) pk_ptr[ch]];
    bits = b[4 * (32 + 64 * (n / 4) + l) + n % 4];
    const unsigned w = (unsigned) (n < 8 ? b[4 * (32 + 64 * 3 + l) + n / 2] : b[2 * l + (n - 8) / 2]);
    return (int) (((n & 1) ? w >> 16 : w & 0xffffu) / 8u) - 512;
  };
  std::vector<int> offs;
  for (size_t ch = 0; ch < nch; ch++)
    for (int l = 0; l < 64; l++) {
      int last = -1024;
      for (int n = 0; n < 12; n++) {
        int bits;
        const int d = entry(ch, l, n, bits);
        if (d == 0) continue;
        if (d <= last) return false;      // the slots keep the row's order only when that order is ascending
        last = d;
        if (std::find(offs.begin(), offs.end(), d) == offs.end()) {
          if ((int) offs.size() == kPkTplSlots) return false;
          offs.push_back(d);
        }
      }
    }
  std::sort(offs.begin(), offs.end());
  std::vector<int> out((size_t) 4 * kPkTplBatchInt4 * nch, 0), ptr(nch, 0);
  for (size_t ch = 0; ch < nch; ch++) {
    ptr[ch] = (int) (kPkTplBatchInt4 * ch);
    for (int l = 0; l < 64; l++)
      for (int n = 0; n < 12; n++) {
        int bits;
        const int d = entry(ch, l, n, bits);
        if (d == 0) continue;
        const int j = (int) (std::lower_bound(offs.begin(), offs.end(), d) - offs.begin());
        out[4 * ((size_t) ptr[ch] + 64 * (j / 4) + l) + j % 4] = bits;
      }
  }
  tpl_reach = 0;
  for (int j = 0; j < kPkTplSlots; j++) {
    tpl_off[j] = j < (int) offs.size() ? offs[j] : 0;
    tpl_reach = std::max(tpl_reach, std::abs(tpl_off[j]));
  }
  pk.swap(out); pk_ptr.swap(ptr);
  tpl = true;
  return true;
}

}  // namespace dc
