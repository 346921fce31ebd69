// tools/tokenise_host/check.py --sanitize: the tokenise kernel on the host under AddressSanitizer + UBSan, shapes the host side rejects
#include "a/b/tokenise.cpp"
#include <cstdio>
#include <random>
int main() {
    std::mt19937 g(1);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    // drawings: 0 lines, 1, 300 (does not fit S below), 1024, 1500 (beyond the kernel's maximum); planks 0, 1, 30 (beyond T), 3, 2
    int nl[5] = {0, 1, 300, 1024, 1500}, np[5] = {0, 1, 30, 3, 2};
    std::vector<int32_t> lo{0}, po{0};
    for (int i = 0; i < 5; ++i) { lo.push_back(lo.back() + nl[i]); po.push_back(po.back() + np[i]); }
    int L = lo.back(), P = po.back();
    std::vector<double> box(4 * L), seg(4 * L), co(6 * P);
    std::vector<uint8_t> vw(L), ty(L);
    std::vector<int32_t> at(6 * P, -1);
    for (auto& v : box) v = u(g);
    for (auto& v : seg) v = u(g);
    for (auto& v : co) v = u(g);
    for (int i = 0; i < L; ++i) { vw[i] = g() % 3; ty[i] = g() % 2; }
    for (int i = 6; i < 6 * P; i += 5) at[i] = i % 6;
    int32_t index[8] = {0, 1, 2, 3, 4, -1, 5, 2000000000};
    for (int S : {4099, 121, 1}) for (int T : {128, 7, 1}) for (int aug : {0, 1}) {
        const int B = 8;
        std::vector<int64_t> iv(B * S), ip(B * S), ic(B * S), iw(B * S), it(B * S), ov(B * T), ol(B * T);
        std::vector<uint8_t> im(B * S), om(B * T);
        std::vector<int32_t> nt(B);
        int rc = pa_tokenise_drawings(lo.data(), box.data(), seg.data(), vw.data(), ty.data(), po.data(), co.data(), at.data(), 5, index, B, S, T,
                                      9, 512, 513, 514, 1, aug, 1.0, 0.9, 0.5, 3, 2, iv.data(), ip.data(), ic.data(), iw.data(), it.data(), im.data(),
                                      ov.data(), ol.data(), om.data(), nt.data(), nullptr);
        long sum = 0; for (int b = 0; b < B; ++b) sum += nt[b];
        printf("S %d T %d aug %d rc %d n_tokens sum %ld\n", S, T, aug, rc, sum);
        if (rc) return 1;
    }
    return 0;
}
