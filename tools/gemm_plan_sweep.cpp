// Host soundness of csrc/gemm_plan.hpp (development aid, not part of the test suite): the plan functions alone, built with
// a plain host compiler and the address / undefined-behaviour sanitizers, over shapes up to M = 2^31 - 1 and K = 2^20.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/gemm_plan_sweep.cpp -o /tmp/gemm_plan_sweep && /tmp/gemm_plan_sweep
// Ends with "ok" and exit status 0 when no arithmetic of the tile / round / rows_main computation overflowed and every plan's
// parts add up to M.
#include "../cli-p_amd/csrc/gemm_plan.hpp"
#include <vector>

using namespace clipmi;

static long long checked = 0;
static int check(const GemmPlan& p, int M) {
    ++checked;
    if (p.err) return p.msg[0] ? 0 : 1;
    long long rows = 0;
    if (p.nparts < 1 || p.nparts > 3) return 1;
    for (int i = 0; i < p.nparts; ++i) {
        const GemmPart& q = p.part[i];
        if (q.rows < 1 || (i + 1 < p.nparts && (q.kernel != GK_256P || q.rows % 256 != 0))) return 1;
        if (q.kernel == GK_256P && (q.grid < 1 || q.grid > plan_chip::NUM_CU || q.lds > plan_chip::LDS_BYTES)) return 1;
        rows += q.rows;
    }
    return rows == M ? 0 : 1;
}

int main() {
    std::vector<int> Ms;
    for (int m = -1; m <= 1100; ++m) Ms.push_back(m);
    for (long long k = 1; k * 256 <= 30000; ++k)
        for (int d = -1; d <= 1; ++d) Ms.push_back((int)(k * 256 + d));
    for (int s = 15; s <= 30; ++s)
        for (int d = -1; d <= 1; ++d) Ms.push_back((1 << s) + d);
    for (int d = 0; d < 600; ++d) Ms.push_back(2147483647 - d);
    const int Ns[] = {512, 768, 1024, 1536, 2304, 3072, 4096, 8192, 16384, 640, 2147483392};
    const int Ks[] = {512, 768, 1024, 3072, 4096, 1 << 16, 1 << 20, (1 << 20) + 128, 2147483520, 64, 0};
    GemmKnobs wide;              // the development knobs at their widest
    wide.split = 100;
    int bad = 0;
    for (int N : Ns)
        for (int K : Ks)
            for (int M : Ms)
                for (int epi = -1; epi <= 9; ++epi) {
                    for (int algo = 0; algo <= 5; ++algo)
                        for (int leaf = 0; leaf < 4; ++leaf) {
                            bad += check(gemm_plan(M, N, K, epi, algo, leaf & 1, leaf >> 1, algo == 3 ? 4 : 0), M);
                            if (algo == 0) bad += check(gemm_plan(M, N, K, epi, 0, leaf & 1, leaf >> 1, 0, wide), M);
                        }
                    for (int mx = 0; mx <= 2; ++mx)
                        for (int f = 0; f < 4; ++f) bad += check(gemm_fp8_plan(M, N, K, epi, mx, f & 1, f >> 1), M);
                }
    printf("%lld plans checked, %d inconsistent\n%s\n", checked, bad, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
