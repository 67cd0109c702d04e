/*
 * ORACLE — test infrastructure only (see oracle/__init__.py).  CPU
 * restatement of the tile rasterizer behind include/gsr.h; also bench.py's
 * `cpu_baseline` for the rasterizer microbench (OpenMP over tiles).
 *
 * What it restates: the canonical graphdeco-inria 3DGS rasterizer
 * (Kerbl et al. 2023, "3D Gaussian Splatting for Real-Time Radiance Field
 * Rendering"; github.com/graphdeco-inria/diff-gaussian-rasterization), which
 * the reference consumes as the EXTERNAL, UNPINNED submodule
 * thirdparty/diff-gaussian-rasterization-modified (.gitmodules:10-12, empty
 * in the snapshot).  Reference call sites: cuda_splatting.py:100-125,
 * visualization.py:563-594.  Parity vs the reference CUDA binary: UNPINNED
 * (no source, no tests, no golden outputs exist for this boundary); the
 * boundary INPUTS are pinned by tests/golden/render_boundary.npz captured
 * from the importable reference glue.
 *
 * Algorithm: cull view z <= 0.2; EWA 2-D covariance with the 1.3*tan(fov)
 * Jacobian clamp and +0.3 low-pass; conic; radius ceil(3 sqrt(lambda_max))
 * with lambda from mid +- sqrt(max(0.1, mid^2-det)); ndc2Pix; 16x16 tile
 * rectangle; SH (deg<=3) -> RGB + 0.5 clamped at 0, or colors_precomp;
 * inclusive scan; keys (tile<<32 | depth bits), stable sort; per-pixel front
 * to back blending: power = -0.5(a dx^2 + c dy^2) - b dx dy, skip power > 0,
 * alpha = min(0.99, o e^power), skip alpha < 1/255, stop when
 * T (1-alpha) < 1e-4, C += f alpha T, out = C + T bg.  Backward: reverse
 * replay with T /= (1 - alpha) and the graphdeco chain rule.
 *
 * Same operation order and the same fixed-sequence exp as
 * splatt3r-slam_amd/csrc/raster_math.hpp, compiled with -ffp-contract=off:
 * the forward is bit-comparable with the HIP kernels.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define BX 16
#define BY 16
#define BS 256

static const float SH_C0 = 0.28209479177387814f;
static const float SH_C1 = 0.4886025119029199f;
static const float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                               -1.0925484305920792f, 0.5462742152960396f};
static const float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                               0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                               -0.5900435899266435f};

typedef struct {
  int H, W;
  float tanfovx, tanfovy, scale_modifier;
  int D;
  float bg[3];
  float viewmatrix[16];
  float projmatrix[16];
  float campos[3];
} oracle_cam;

/* The blend's exponential.  Default: the same fixed-sequence Cody-Waite +
 * degree-6 Horner exp as raster_math.hpp (bit-comparable with the HIP
 * kernels; <= 3 ulp from the correctly rounded exp on [-87, 0], about 13 %
 * of those values differ from it, tests/test_raster.py
 * test_oracle_fexp_ulp_bound).  oracle_raster_set_exp(1) switches the oracle
 * to libm expf -- the canonical graphdeco expression `exp(power)` -- so the
 * HIP image can be held to a tolerance against an exponential that is not
 * the kernel's own (test_hip_forward_vs_libm_exp_oracle). */
static int g_libm_exp = 0;

void oracle_raster_set_exp(int libm) { g_libm_exp = libm; }

static float fexp(float x) {
  if (g_libm_exp) return expf(x);
  if (x < -87.0f) return 0.0f;
  float k = rintf(x * 1.44269504088896341f);
  float r = x - k * 0.693145751953125f;
  r = r - k * 1.42860682030941723e-06f;
  float p = 0.00138888888888889f;
  p = p * r + 0.00833333333333333f;
  p = p * r + 0.0416666666666667f;
  p = p * r + 0.166666666666667f;
  p = p * r + 0.5f;
  p = p * r + 1.0f;
  p = p * r + 1.0f;
  return ldexpf(p, (int)k);
}

float oracle_fexp(float x) { return fexp(x); }

static float ndc2pix(float v, int S) { return ((v + 1.0f) * S - 1.0f) * 0.5f; }

static void get_rect(float px, float py, int r, int gx, int gy, int* x0, int* y0, int* x1,
                     int* y1) {
  int a = (int)((px - r) / BX), b = (int)((py - r) / BY);
  int c = (int)((px + r + BX - 1) / BX), d = (int)((py + r + BY - 1) / BY);
  *x0 = a < 0 ? 0 : (a > gx ? gx : a);
  *y0 = b < 0 ? 0 : (b > gy ? gy : b);
  *x1 = c < 0 ? 0 : (c > gx ? gx : c);
  *y1 = d < 0 ? 0 : (d > gy ? gy : d);
}

static void xform43(const float* m, float x, float y, float z, float* o) {
  o[0] = m[0] * x + m[4] * y + m[8] * z + m[12];
  o[1] = m[1] * x + m[5] * y + m[9] * z + m[13];
  o[2] = m[2] * x + m[6] * y + m[10] * z + m[14];
}

static void cov3d_from_scale_rot(const float* s3, float mod, const float* q, float* cov) {
  float r = q[0], x = q[1], y = q[2], z = q[3];
  float R[9] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y),
                2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x),
                2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)};
  float s[3] = {mod * s3[0], mod * s3[1], mod * s3[2]};
  float M[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M[3 * i + j] = R[3 * i + j] * s[j];
  int k = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j)
      cov[k++] = M[3 * i + 0] * M[3 * j + 0] + M[3 * i + 1] * M[3 * j + 1] +
                 M[3 * i + 2] * M[3 * j + 2];
}

typedef struct {
  float T[6];
  float a, b, c, tx, ty, tz, xmul, ymul;
} ewa_t;

static ewa_t ewa(float mx, float my, float mz, const float* cov3, const float* vm, float fx,
                 float fy, float tanfx, float tanfy) {
  ewa_t e;
  float t[3];
  xform43(vm, mx, my, mz, t);
  const float limx = 1.3f * tanfx, limy = 1.3f * tanfy;
  const float txtz = t[0] / t[2], tytz = t[1] / t[2];
  e.xmul = (txtz < -limx || txtz > limx) ? 0.0f : 1.0f;
  e.ymul = (tytz < -limy || tytz > limy) ? 0.0f : 1.0f;
  e.tx = fminf(limx, fmaxf(-limx, txtz)) * t[2];
  e.ty = fminf(limy, fmaxf(-limy, tytz)) * t[2];
  e.tz = t[2];
  const float J00 = fx / e.tz, J02 = -(fx * e.tx) / (e.tz * e.tz);
  const float J11 = fy / e.tz, J12 = -(fy * e.ty) / (e.tz * e.tz);
  for (int c = 0; c < 3; ++c) {
    e.T[c] = J00 * vm[0 + 4 * c] + J02 * vm[2 + 4 * c];
    e.T[3 + c] = J11 * vm[1 + 4 * c] + J12 * vm[2 + 4 * c];
  }
  const float V[9] = {cov3[0], cov3[1], cov3[2], cov3[1], cov3[3], cov3[4],
                      cov3[2], cov3[4], cov3[5]};
  float TV0[3], TV1[3];
  for (int c = 0; c < 3; ++c) {
    TV0[c] = e.T[0] * V[c] + e.T[1] * V[3 + c] + e.T[2] * V[6 + c];
    TV1[c] = e.T[3] * V[c] + e.T[4] * V[3 + c] + e.T[5] * V[6 + c];
  }
  e.a = TV0[0] * e.T[0] + TV0[1] * e.T[1] + TV0[2] * e.T[2];
  e.b = TV0[0] * e.T[3] + TV0[1] * e.T[4] + TV0[2] * e.T[5];
  e.c = TV1[0] * e.T[3] + TV1[1] * e.T[4] + TV1[2] * e.T[5];
  return e;
}

static void sh_basis(int deg, float x, float y, float z, float* B) {
  B[0] = SH_C0;
  if (deg > 0) {
    B[1] = -SH_C1 * y; B[2] = SH_C1 * z; B[3] = -SH_C1 * x;
    if (deg > 1) {
      float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
      B[4] = SH_C2[0] * xy; B[5] = SH_C2[1] * yz; B[6] = SH_C2[2] * (2.0f * zz - xx - yy);
      B[7] = SH_C2[3] * xz; B[8] = SH_C2[4] * (xx - yy);
      if (deg > 2) {
        B[9] = SH_C3[0] * y * (3.0f * xx - yy);
        B[10] = SH_C3[1] * xy * z;
        B[11] = SH_C3[2] * y * (4.0f * zz - xx - yy);
        B[12] = SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
        B[13] = SH_C3[4] * x * (4.0f * zz - xx - yy);
        B[14] = SH_C3[5] * z * (xx - yy);
        B[15] = SH_C3[6] * x * (xx - 3.0f * yy);
      }
    }
  }
}

typedef struct {
  uint64_t key;
  uint32_t val;
  uint32_t pos;
} inst_t;

static int cmp_inst(const void* a, const void* b) {
  const inst_t* x = (const inst_t*)a;
  const inst_t* y = (const inst_t*)b;
  if (x->key != y->key) return x->key < y->key ? -1 : 1;
  return x->pos < y->pos ? -1 : (x->pos > y->pos);
}

/*
 * Forward (+ optional backward when dL_dout != NULL).  Arrays as in gsr.h.
 * Returns num_rendered.  Gradient outputs may be NULL when not wanted.
 */
int64_t oracle_raster(const oracle_cam* cam, int64_t P, int M, const float* means,
                      const float* scales, const float* rots, const float* cov_pre,
                      const float* shs, const float* colors_pre, const float* opac,
                      float* out_color, int32_t* radii, const float* dL_dout,
                      float* dL_dmeans2D, float* dL_dconic, float* dL_dopacity,
                      float* dL_dcolors, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                      int nthreads) {
  const int W = cam->W, H = cam->H;
  const int gx = (W + BX - 1) / BX, gy = (H + BY - 1) / BY, ntiles = gx * gy;
  const float fx = W / (2.0f * cam->tanfovx), fy = H / (2.0f * cam->tanfovy);
  const float* vm = cam->viewmatrix;
  const float* pm = cam->projmatrix;
  memset(out_color, 0, sizeof(float) * 3 * (size_t)H * W);
  if (P == 0) return 0;
  float* depth = (float*)malloc(sizeof(float) * P);
  float* rec = (float*)malloc(sizeof(float) * P * 8); /* x y ca cb cc o */
  float* rgb = (float*)malloc(sizeof(float) * P * 3);
  float* cov3s = (float*)malloc(sizeof(float) * P * 6);
  uint8_t* clamped = (uint8_t*)calloc(P * 3, 1);
  uint32_t* tiles = (uint32_t*)calloc(P, sizeof(uint32_t));
  uint64_t* offsets = (uint64_t*)malloc(sizeof(uint64_t) * P);

#pragma omp parallel for num_threads(nthreads) schedule(static)
  for (int64_t i = 0; i < P; ++i) {
    radii[i] = 0;
    tiles[i] = 0;
    const float mx = means[i * 3], my = means[i * 3 + 1], mz = means[i * 3 + 2];
    float pv[3];
    xform43(vm, mx, my, mz, pv);
    if (pv[2] <= 0.2f) continue;
    float ph[4];
    xform43(pm, mx, my, mz, ph);
    ph[3] = pm[3] * mx + pm[7] * my + pm[11] * mz + pm[15];
    const float pw = 1.0f / (ph[3] + 0.0000001f);
    const float ppx = ph[0] * pw, ppy = ph[1] * pw;
    float* cov3 = cov3s + i * 6;
    if (cov_pre)
      for (int k = 0; k < 6; ++k) cov3[k] = cov_pre[i * 6 + k];
    else
      cov3d_from_scale_rot(scales + i * 3, cam->scale_modifier, rots + i * 4, cov3);
    ewa_t e = ewa(mx, my, mz, cov3, vm, fx, fy, cam->tanfovx, cam->tanfovy);
    const float a = e.a + 0.3f, b = e.b, c = e.c + 0.3f;
    const float det = a * c - b * b;
    if (det == 0.0f) continue;
    const float det_inv = 1.0f / det;
    const float mid = 0.5f * (a + c);
    const float disc = sqrtf(fmaxf(0.1f, mid * mid - det));
    const float l1 = mid + disc, l2 = mid - disc;
    const int r = (int)ceilf(3.0f * sqrtf(fmaxf(l1, l2)));
    const float px = ndc2pix(ppx, W), py = ndc2pix(ppy, H);
    int x0, y0, x1, y1;
    get_rect(px, py, r, gx, gy, &x0, &y0, &x1, &y1);
    if ((x1 - x0) * (y1 - y0) == 0) continue;
    if (colors_pre) {
      for (int ch = 0; ch < 3; ++ch) rgb[i * 3 + ch] = colors_pre[i * 3 + ch];
    } else {
      float dx = mx - cam->campos[0], dy = my - cam->campos[1], dz = mz - cam->campos[2];
      float len = sqrtf(dx * dx + dy * dy + dz * dz);
      dx = dx / len; dy = dy / len; dz = dz / len;
      float B[16];
      sh_basis(cam->D, dx, dy, dz, B);
      const int nb = (cam->D + 1) * (cam->D + 1);
      const float* sh = shs + i * (int64_t)M * 3;
      for (int ch = 0; ch < 3; ++ch) {
        float acc = B[0] * sh[ch];
        for (int k = 1; k < nb; ++k) acc = acc + B[k] * sh[k * 3 + ch];
        acc = acc + 0.5f;
        clamped[i * 3 + ch] = acc < 0.0f;
        rgb[i * 3 + ch] = fmaxf(acc, 0.0f);
      }
    }
    depth[i] = pv[2];
    radii[i] = r;
    float* R8 = rec + i * 8;
    R8[0] = px; R8[1] = py; R8[2] = c * det_inv; R8[3] = -b * det_inv; R8[4] = a * det_inv;
    R8[5] = opac[i];
    tiles[i] = (uint32_t)((y1 - y0) * (x1 - x0));
  }
  uint64_t run = 0;
  for (int64_t i = 0; i < P; ++i) { run += tiles[i]; offsets[i] = run; }
  const int64_t R = (int64_t)run;
  inst_t* inst = (inst_t*)malloc(sizeof(inst_t) * (R > 0 ? R : 1));
#pragma omp parallel for num_threads(nthreads) schedule(static)
  for (int64_t i = 0; i < P; ++i) {
    if (radii[i] <= 0) continue;
    uint64_t off = i == 0 ? 0 : offsets[i - 1];
    int x0, y0, x1, y1;
    get_rect(rec[i * 8], rec[i * 8 + 1], radii[i], gx, gy, &x0, &y0, &x1, &y1);
    uint32_t dbits;
    memcpy(&dbits, &depth[i], 4);
    for (int y = y0; y < y1; ++y)
      for (int x = x0; x < x1; ++x) {
        inst[off].key = ((uint64_t)(y * gx + x) << 32) | dbits;
        inst[off].val = (uint32_t)i;
        inst[off].pos = (uint32_t)off;
        ++off;
      }
  }
  qsort(inst, R, sizeof(inst_t), cmp_inst);
  int64_t* rs = (int64_t*)calloc(ntiles, sizeof(int64_t));
  int64_t* re = (int64_t*)calloc(ntiles, sizeof(int64_t));
  for (int64_t k = 0; k < R; ++k) {
    uint32_t t = (uint32_t)(inst[k].key >> 32);
    if (k == 0 || (uint32_t)(inst[k - 1].key >> 32) != t) rs[t] = k;
    re[t] = k + 1;
  }
  float* finalT = (float*)malloc(sizeof(float) * (size_t)H * W);
  uint32_t* ncontrib = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)H * W);

#pragma omp parallel for num_threads(nthreads) schedule(dynamic, 4)
  for (int tile = 0; tile < ntiles; ++tile) {
    const int tx = tile % gx, ty = tile / gx;
    for (int ly = 0; ly < BY; ++ly)
      for (int lx = 0; lx < BX; ++lx) {
        const int px = tx * BX + lx, py = ty * BY + ly;
        if (px >= W || py >= H) continue;
        const float pxf = (float)px, pyf = (float)py;
        float T = 1.0f;
        uint32_t contributor = 0, last = 0;
        float C[3] = {0.f, 0.f, 0.f};
        for (int64_t k = rs[tile]; k < re[tile]; ++k) {
          ++contributor;
          const uint32_t id = inst[k].val;
          const float* q = rec + (int64_t)id * 8;
          const float dx = q[0] - pxf, dy = q[1] - pyf;
          const float power = -0.5f * (q[2] * dx * dx + q[4] * dy * dy) - q[3] * dx * dy;
          if (power > 0.0f) continue;
          const float alpha = fminf(0.99f, q[5] * fexp(power));
          if (alpha < 1.0f / 255.0f) continue;
          const float test_T = T * (1.0f - alpha);
          if (test_T < 0.0001f) break; /* "done": no later Gaussian contributes */
          for (int ch = 0; ch < 3; ++ch) C[ch] = C[ch] + rgb[id * 3 + ch] * alpha * T;
          T = test_T;
          last = contributor;
        }
        const int pid = py * W + px;
        finalT[pid] = T;
        ncontrib[pid] = last;
        for (int ch = 0; ch < 3; ++ch) out_color[ch * H * W + pid] = C[ch] + T * cam->bg[ch];
      }
  }

  if (dL_dout) {
    float* dconic = dL_dconic ? dL_dconic : (float*)calloc(P * 4, sizeof(float));
    memset(dconic, 0, sizeof(float) * P * 4);
    memset(dL_dmeans2D, 0, sizeof(float) * P * 3);
    memset(dL_dopacity, 0, sizeof(float) * P);
    memset(dL_dcolors, 0, sizeof(float) * P * 3);
    memset(dL_dmeans3D, 0, sizeof(float) * P * 3);
    memset(dL_dcov3D, 0, sizeof(float) * P * 6);
    if (dL_dsh) memset(dL_dsh, 0, sizeof(float) * P * M * 3);
    const float ddelx_dx = 0.5f * W, ddely_dy = 0.5f * H;
    for (int tile = 0; tile < ntiles; ++tile) {
      const int tx = tile % gx, ty = tile / gx;
      for (int ly = 0; ly < BY; ++ly)
        for (int lx = 0; lx < BX; ++lx) {
          const int px = tx * BX + lx, py = ty * BY + ly;
          if (px >= W || py >= H) continue;
          const int pid = py * W + px;
          const float pxf = (float)px, pyf = (float)py;
          const float T_final = finalT[pid];
          float T = T_final;
          uint32_t contributor = (uint32_t)(re[tile] - rs[tile]);
          const uint32_t last = ncontrib[pid];
          float dpix[3];
          for (int ch = 0; ch < 3; ++ch) dpix[ch] = dL_dout[ch * H * W + pid];
          const float bg_dot = cam->bg[0] * dpix[0] + cam->bg[1] * dpix[1] + cam->bg[2] * dpix[2];
          float acc[3] = {0, 0, 0}, lc[3] = {0, 0, 0}, last_alpha = 0.f;
          for (int64_t k = re[tile] - 1; k >= rs[tile]; --k) {
            --contributor;
            if (contributor >= last) continue;
            const uint32_t id = inst[k].val;
            const float* q = rec + (int64_t)id * 8;
            const float dx = q[0] - pxf, dy = q[1] - pyf;
            const float power = -0.5f * (q[2] * dx * dx + q[4] * dy * dy) - q[3] * dx * dy;
            if (power > 0.0f) continue;
            const float G = fexp(power);
            const float alpha = fminf(0.99f, q[5] * G);
            if (alpha < 1.0f / 255.0f) continue;
            T = T / (1.0f - alpha);
            const float dchannel_dcolor = alpha * T;
            float dL_dalpha = 0.f;
            for (int ch = 0; ch < 3; ++ch) {
              const float cc = rgb[id * 3 + ch];
              acc[ch] = last_alpha * lc[ch] + (1.0f - last_alpha) * acc[ch];
              lc[ch] = cc;
              dL_dalpha = dL_dalpha + (cc - acc[ch]) * dpix[ch];
              dL_dcolors[id * 3 + ch] += dchannel_dcolor * dpix[ch];
            }
            dL_dalpha = dL_dalpha * T;
            last_alpha = alpha;
            dL_dalpha = dL_dalpha + (-T_final / (1.0f - alpha)) * bg_dot;
            const float dL_dG = q[5] * dL_dalpha;
            const float gdx = G * dx, gdy = G * dy;
            const float dG_ddelx = -gdx * q[2] - gdy * q[3];
            const float dG_ddely = -gdy * q[4] - gdx * q[3];
            dL_dmeans2D[id * 3 + 0] += dL_dG * dG_ddelx * ddelx_dx;
            dL_dmeans2D[id * 3 + 1] += dL_dG * dG_ddely * ddely_dy;
            dconic[id * 4 + 0] += -0.5f * gdx * dx * dL_dG;
            dconic[id * 4 + 1] += -0.5f * gdx * dy * dL_dG;
            dconic[id * 4 + 3] += -0.5f * gdy * dy * dL_dG;
            dL_dopacity[id] += G * dL_dalpha;
          }
        }
    }
    for (int64_t i = 0; i < P; ++i) {
      if (!(radii[i] > 0)) continue;
      const float mx = means[i * 3], my = means[i * 3 + 1], mz = means[i * 3 + 2];
      const float* cov3 = cov3s + i * 6;
      ewa_t e = ewa(mx, my, mz, cov3, vm, fx, fy, cam->tanfovx, cam->tanfovy);
      const float a = e.a + 0.3f, b = e.b, c = e.c + 0.3f;
      const float dcx = dconic[i * 4], dcy = dconic[i * 4 + 1], dcz = dconic[i * 4 + 3];
      const float denom = a * c - b * b;
      const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
      float da = 0, db = 0, dc = 0;
      const float* T6 = e.T;
      float* dcov = dL_dcov3D + i * 6;
      if (denom2inv != 0.0f) {
        da = denom2inv * (-c * c * dcx + 2.0f * b * c * dcy + (denom - a * c) * dcz);
        dc = denom2inv * (-a * a * dcz + 2.0f * a * b * dcy + (denom - a * c) * dcx);
        db = denom2inv * 2.0f * (b * c * dcx - (denom + 2.0f * b * b) * dcy + a * b * dcz);
        dcov[0] = T6[0] * T6[0] * da + T6[0] * T6[3] * db + T6[3] * T6[3] * dc;
        dcov[3] = T6[1] * T6[1] * da + T6[1] * T6[4] * db + T6[4] * T6[4] * dc;
        dcov[5] = T6[2] * T6[2] * da + T6[2] * T6[5] * db + T6[5] * T6[5] * dc;
        dcov[1] = 2.0f * T6[0] * T6[1] * da + (T6[0] * T6[4] + T6[1] * T6[3]) * db + 2.0f * T6[3] * T6[4] * dc;
        dcov[2] = 2.0f * T6[0] * T6[2] * da + (T6[0] * T6[5] + T6[2] * T6[3]) * db + 2.0f * T6[3] * T6[5] * dc;
        dcov[4] = 2.0f * T6[2] * T6[1] * da + (T6[1] * T6[5] + T6[2] * T6[4]) * db + 2.0f * T6[4] * T6[5] * dc;
      }
      const float V[9] = {cov3[0], cov3[1], cov3[2], cov3[1], cov3[3], cov3[4],
                          cov3[2], cov3[4], cov3[5]};
      float dT0[3], dT1[3];
      for (int k = 0; k < 3; ++k) {
        const float t0v = T6[0] * V[k] + T6[1] * V[3 + k] + T6[2] * V[6 + k];
        const float t1v = T6[3] * V[k] + T6[4] * V[3 + k] + T6[5] * V[6 + k];
        dT0[k] = 2.0f * t0v * da + t1v * db;
        dT1[k] = 2.0f * t1v * dc + t0v * db;
      }
      const float dJ00 = vm[0] * dT0[0] + vm[4] * dT0[1] + vm[8] * dT0[2];
      const float dJ02 = vm[2] * dT0[0] + vm[6] * dT0[1] + vm[10] * dT0[2];
      const float dJ11 = vm[1] * dT1[0] + vm[5] * dT1[1] + vm[9] * dT1[2];
      const float dJ12 = vm[2] * dT1[0] + vm[6] * dT1[1] + vm[10] * dT1[2];
      const float tz = 1.0f / e.tz, tz2 = tz * tz, tz3 = tz2 * tz;
      const float dtx = e.xmul * -fx * tz2 * dJ02;
      const float dty = e.ymul * -fy * tz2 * dJ12;
      const float dtz = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + (2.0f * fx * e.tx) * tz3 * dJ02 +
                        (2.0f * fy * e.ty) * tz3 * dJ12;
      float gmx = vm[0] * dtx + vm[1] * dty + vm[2] * dtz;
      float gmy = vm[4] * dtx + vm[5] * dty + vm[6] * dtz;
      float gmz = vm[8] * dtx + vm[9] * dty + vm[10] * dtz;
      float ph3 = pm[3] * mx + pm[7] * my + pm[11] * mz + pm[15];
      const float mw = 1.0f / (ph3 + 0.0000001f);
      const float mul1 = (pm[0] * mx + pm[4] * my + pm[8] * mz + pm[12]) * mw * mw;
      const float mul2 = (pm[1] * mx + pm[5] * my + pm[9] * mz + pm[13]) * mw * mw;
      const float d2x = dL_dmeans2D[i * 3], d2y = dL_dmeans2D[i * 3 + 1];
      gmx = gmx + ((pm[0] * mw - pm[3] * mul1) * d2x + (pm[1] * mw - pm[3] * mul2) * d2y);
      gmy = gmy + ((pm[4] * mw - pm[7] * mul1) * d2x + (pm[5] * mw - pm[7] * mul2) * d2y);
      gmz = gmz + ((pm[8] * mw - pm[11] * mul1) * d2x + (pm[9] * mw - pm[11] * mul2) * d2y);
      if (shs && dL_dsh) {
        const float ox = mx - cam->campos[0], oy = my - cam->campos[1], oz = mz - cam->campos[2];
        const float len = sqrtf(ox * ox + oy * oy + oz * oz);
        float B[16];
        sh_basis(cam->D, ox / len, oy / len, oz / len, B);
        const int nb = (cam->D + 1) * (cam->D + 1);
        for (int k = 0; k < nb && k < M; ++k)
          for (int ch = 0; ch < 3; ++ch)
            dL_dsh[(i * M + k) * 3 + ch] =
                B[k] * (clamped[i * 3 + ch] ? 0.0f : dL_dcolors[i * 3 + ch]);
        /* degree-0 has no view-direction term; for higher degrees dL_dmeans3D
           of the kernels is checked against float64 autograd
           (tests/test_raster_grad.py
           test_hip_backward_vs_float64_reference), not restated here */
      }
      dL_dmeans3D[i * 3] = gmx;
      dL_dmeans3D[i * 3 + 1] = gmy;
      dL_dmeans3D[i * 3 + 2] = gmz;
    }
    if (!dL_dconic) free(dconic);
  }
  free(depth); free(rec); free(rgb); free(cov3s); free(clamped); free(tiles); free(offsets);
  free(inst); free(rs); free(re); free(finalT); free(ncontrib);
  return R;
}
