// Where does the signed error of the forced path's log p come from?  csrc/decode.hip forms
//   p = expf(v - vmax) / vsum [* (1 - prob)],  lp = logf(p)
// in f32.  This program evaluates, with the library's compile flags, on the device and against double arithmetic on the host:
//   1. logf(p) alone, p log-uniform in [1e-16, 1): error against log of THE SAME f32 p, in ulps of the result;
//   2. expf(x) alone, x uniform in [-37, 0): relative error in ulps of the result;
//   3. the chain logf(expf(x) / s), s uniform in [1, 50): error against x - log(s), absolute, by octave of |log p|.
// hipcc --offload-arch=gfx950 -O3 logf_bias.hip -o logf_bias
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

__global__ void eval(const float* p, const float* x, const float* s, float* lg, float* ex, float* chain, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    lg[i] = logf(p[i]);
    ex[i] = expf(x[i]);
    chain[i] = logf(expf(x[i]) / s[i]);
}

static double ulp_of(double v) { int e; frexp(fabs(v), &e); return ldexp(1.0, e - 24); }

int main() {
    const int n = 1 << 20;
    std::vector<float> p(n), x(n), s(n), lg(n), ex(n), ch(n);
    srand(7);
    auto u = [] { return (rand() + 0.5) / ((double)RAND_MAX + 1.0); };
    for (int i = 0; i < n; ++i) { p[i] = (float)exp(-36.8 * u()); x[i] = (float)(-37.0 * u()); s[i] = (float)(1.0 + 49.0 * u()); }
    float *dp, *dx, *ds, *dl, *de, *dc;
    const size_t b = n * sizeof(float);
    if (hipMalloc(&dp, b) || hipMalloc(&dx, b) || hipMalloc(&ds, b) || hipMalloc(&dl, b) || hipMalloc(&de, b) || hipMalloc(&dc, b)) return 1;
    hipMemcpy(dp, p.data(), b, hipMemcpyHostToDevice); hipMemcpy(dx, x.data(), b, hipMemcpyHostToDevice); hipMemcpy(ds, s.data(), b, hipMemcpyHostToDevice);
    eval<<<(n + 255) / 256, 256>>>(dp, dx, ds, dl, de, dc, n);
    if (hipDeviceSynchronize() != hipSuccess) return 2;
    hipMemcpy(lg.data(), dl, b, hipMemcpyDeviceToHost); hipMemcpy(ex.data(), de, b, hipMemcpyDeviceToHost); hipMemcpy(ch.data(), dc, b, hipMemcpyDeviceToHost);
    const int NO = 6;                                   // octaves of |log p|: [1,2) [2,4) ... [32,64)
    double sl[NO] = {0}, al[NO] = {0}, ml[NO] = {0}, sc[NO] = {0}, ac[NO] = {0}; long cl[NO] = {0}, cc[NO] = {0}, exact[NO] = {0};
    double se = 0, ae = 0, me = 0;
    for (int i = 0; i < n; ++i) {
        const double want = log((double)p[i]);
        int o = (int)floor(log2(fabs(want)));
        if (o >= 0 && o < NO) {
            const double e = ((double)lg[i] - want) / ulp_of(want);
            sl[o] += e; al[o] += fabs(e); ml[o] = fmax(ml[o], fabs(e)); ++cl[o];
            exact[o] += lg[i] == (float)want;
        }
        const double we = exp((double)x[i]), ee = ((double)ex[i] - we) / ulp_of(we);
        se += ee; ae += fabs(ee); me = fmax(me, fabs(ee));
        const double wc = (double)x[i] - log((double)s[i]);
        o = (int)floor(log2(fabs(wc)));
        if (o >= 0 && o < NO) { sc[o] += (double)ch[i] - wc; ac[o] += fabs((double)ch[i] - wc); ++cc[o]; }
    }
    printf("1. logf(p) against log of the same f32 p, in ulps of the result, by |log p| in [x, 2x):\n");
    for (int o = 0; o < NO; ++o) if (cl[o])
        printf("   %2d: signed mean %+.4f  mean |.| %.4f  max %.3f  correctly rounded %.1f %%  (n %ld)\n", 1 << o, sl[o] / cl[o], al[o] / cl[o], ml[o], 100.0 * exact[o] / cl[o], cl[o]);
    printf("2. expf(x), x in [-37, 0), in ulps of the result: signed mean %+.4f  mean |.| %.4f  max %.3f\n", se / n, ae / n, me);
    printf("3. logf(expf(x) / s) against x - log(s), absolute, by |log p| in [x, 2x):\n");
    for (int o = 0; o < NO; ++o) if (cc[o])
        printf("   %2d: signed mean %+.3e  mean |.| %.3e  (one ulp of the result: %.2e; n %ld)\n", 1 << o, sc[o] / cc[o], ac[o] / cc[o], ldexp(1.0, o - 23), cc[o]);
    return 0;
}
