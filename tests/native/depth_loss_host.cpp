// Host restatement of the depth loss: runs depth_loss_math.hpp's s3z::pixel /
// terms / pair_term / dl_dr / grads, the functions the kernels of
// depth_loss.hip call, on the CPU (tests/test_depth_loss.py), tile by tile in
// the kernel's order: a tile's pixels, then its pairs, then the tiles of an
// image in order.  Host code built with -ffp-contract=off.
//
//   depth_loss_host IN OUT B H W HAS_W HAS_S ALPHA_MIN
//     IN:  depth, alpha, target [B, H, W] float32, weight [B, H, W] if HAS_W,
//          scale [B] if HAS_S, coef [B, 3] float32
//     OUT: sums [B, S3Z_NSUMS] float64, rmap, grad_depth, grad_alpha
//          [B, H, W] float32
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "depth_loss_math.hpp"

static std::vector<char> read_all(const char* path) {
  std::vector<char> v;
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  char buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

template <typename T>
static void put(FILE* f, const std::vector<T>& v) {
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror("write"); exit(2); }
}

int main(int argc, char** argv) {
  if (argc != 9) {
    fprintf(stderr, "usage: see the head of tests/native/depth_loss_host.cpp\n");
    return 2;
  }
  const int B = atoi(argv[3]), H = atoi(argv[4]), W = atoi(argv[5]);
  const bool has_w = atoi(argv[6]) != 0, has_s = atoi(argv[7]) != 0;
  const double alpha_min = strtod(argv[8], nullptr);
  if (B < 1 || H < 1 || W < 1) return 2;
  const size_t n = (size_t)B * H * W, plane = (size_t)H * W;
  const std::vector<char> in = read_all(argv[1]);
  const size_t floats = n * (3 + (has_w ? 1 : 0)) + (has_s ? B : 0) + (size_t)B * 3;
  if (in.size() != floats * 4) {
    fprintf(stderr, "depth_loss_host: %zu input bytes, expected %zu\n", in.size(), floats * 4);
    return 2;
  }
  std::vector<float> all(floats);
  memcpy(all.data(), in.data(), in.size());
  const float* depth = all.data();
  const float* alpha = depth + n;
  const float* target = alpha + n;
  const float* weight = has_w ? target + n : nullptr;
  const float* scale = has_s ? target + n * (has_w ? 2 : 1) : nullptr;
  const float* coef = all.data() + floats - (size_t)B * 3;

  std::vector<double> sums((size_t)B * S3Z_NSUMS, 0.0);
  std::vector<float> rmap(n), gd(n, 0.f), ga(n, 0.f);
  std::vector<s3z::Pixel> px(n);
  for (int b = 0; b < B; ++b) {
    const double s = scale ? (double)scale[b] : 1.0;
    for (size_t i = b * plane; i < (b + 1) * plane; ++i) {
      px[i] = s3z::pixel(depth[i], alpha[i], target[i], weight ? weight[i] : 1.f, s, alpha_min);
      rmap[i] = (float)px[i].r;
    }
  }
  const s3z::Pixel none{0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < B; ++b) {
    const double s = scale ? (double)scale[b] : 1.0;
    const double c_abs = coef[b * 3], c_sq = coef[b * 3 + 1], c_grad = coef[b * 3 + 2];
    const s3z::Pixel* P = &px[b * plane];
    auto at = [&](int y, int x) -> const s3z::Pixel& {
      return (y >= 0 && y < H && x >= 0 && x < W) ? P[(size_t)y * W + x] : none;
    };
    double* S = &sums[(size_t)b * S3Z_NSUMS];
    for (int y0 = 0; y0 < H; y0 += S3Z_TILE_H)
      for (int x0 = 0; x0 < W; x0 += S3Z_TILE_W) {
        double part[S3Z_NSUMS] = {0.0};
        const int y1 = y0 + S3Z_TILE_H < H ? y0 + S3Z_TILE_H : H;
        const int x1 = x0 + S3Z_TILE_W < W ? x0 + S3Z_TILE_W : W;
        for (int y = y0; y < y1; ++y)
          for (int x = x0; x < x1; ++x) {
            const s3z::Pixel& p = at(y, x);
            if (!(p.w > 0.0)) continue;
            double t[S3Z_NSUMS];
            s3z::terms(p, target[b * plane + (size_t)y * W + x], t);
            for (int k = 0; k < S3Z_NSUMS; ++k) part[k] += t[k];
          }
        for (int y = y0; y < y1; ++y)
          for (int x = x0; x < x1; ++x) {
            const s3z::Pixel& p = at(y, x);
            if (!(p.w > 0.0)) continue;
            const s3z::Pixel& r = at(y, x + 1);
            const s3z::Pixel& d = at(y + 1, x);
            if (r.w > 0.0) {
              part[S3Z_SUM_GRAD] += s3z::pair_term(p.w, p.r, r.w, r.r);
              part[S3Z_SUM_WG] += s3z::pair_weight(p.w, r.w);
            }
            if (d.w > 0.0) {
              part[S3Z_SUM_GRAD] += s3z::pair_term(p.w, p.r, d.w, d.r);
              part[S3Z_SUM_WG] += s3z::pair_weight(p.w, d.w);
            }
          }
        for (int k = 0; k < S3Z_NSUMS; ++k) S[k] += part[k];
      }
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const s3z::Pixel& p = at(y, x);
        if (!(p.w > 0.0)) continue;
        const s3z::Pixel &l = at(y, x - 1), &r = at(y, x + 1), &u = at(y - 1, x), &d = at(y + 1, x);
        const double g = s3z::dl_dr(p.w, p.r, l.w, l.r, r.w, r.r, u.w, u.r, d.w, d.r, c_abs, c_sq,
                                    c_grad);
        const size_t i = b * plane + (size_t)y * W + x;
        s3z::grads(g, depth[i], alpha[i], s, gd[i], ga[i]);
      }
  }
  FILE* f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  put(f, sums);
  put(f, rmap);
  put(f, gd);
  put(f, ga);
  fclose(f);
  return 0;
}
