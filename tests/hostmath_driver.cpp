// Stand-alone driver of starfish_amd/csrc/sf_hostmath.cpp for tests/test_hostmath.py (host compiler, no HIP).
// usage: hostmath_driver <lu|inv|emu|ext|tw|grid|band> with the numbers on stdin (strtod: hex floats are exact); prints
// "rc <code>", "err <text of sf_last_error()>", then one "<name> <hex floats...>" line per result.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sf_band_shape.h"
#include "sf_hostmath.h"

static double next_double() {
    char tok[128];
    if (scanf("%127s", tok) != 1) {
        fprintf(stderr, "hostmath_driver: input ended early\n");
        exit(2);
    }
    return strtod(tok, nullptr);
}
static std::vector<double> next_vector(size_t n) {
    std::vector<double> v(n);
    for (double& x : v) x = next_double();
    return v;
}
static void put(const char* name, const std::vector<double>& v) {
    printf("%s", name);
    for (double x : v) printf(" %a", x);
    printf("\n");
}
static int done(int rc) {
    printf("rc %d\nerr %s\n", rc, rc ? sf_last_error() : "");
    return 0;
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "lu" || cmd == "inv") {
        const int n = (int)next_double();
        const std::vector<double> x = next_vector(n > 0 ? n : 0);
        std::vector<double> t, Lf, Uf, rdiag;
        const int rc = quintic_collocation_lu(x.data(), n, t, Lf, Uf, rdiag);
        done(rc);
        if (rc) return 0;
        if (cmd == "lu") {
            put("t", t);
            put("Lf", Lf);
            put("Uf", Uf);
            put("rdiag", rdiag);
            return 0;
        }
        // c = A^-1 y with the truncated inverse: once from the plain band, once from its 16 x 16 blocks, both summing
        // over the columns in ascending order
        const std::vector<double> y = next_vector(n);
        std::vector<double> band, tblk, c_band(n, 0.0), c_blocks(n, 0.0);
        truncated_inverse_band(n, Lf, Uf, rdiag, band);
        inverse_band_blocks(n, band, tblk);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                if (j - i <= SF_IW && i - j <= SF_IW) c_band[i] += band[(size_t)(j - i + SF_IW) * n + i] * y[j];
        const int nkb = 2 * (SF_IW / 16) + 1;
        for (int ib = 0; ib < n / 16; ++ib)
            for (int kb = 0; kb < nkb; ++kb)
                for (int cc = 0; cc < 16; ++cc) {
                    const int k = (ib - SF_IW / 16 + kb) * 16 + cc;
                    if (k < 0 || k >= n) continue;
                    for (int r = 0; r < 16; ++r) c_blocks[ib * 16 + r] += tblk[(((size_t)ib * nkb + kb) * 16 + r) * 16 + cc] * y[k];
                }
        put("c_band", c_band);
        put("c_blocks", c_blocks);
        put("sizes", {(double)band.size(), (double)tblk.size()});
    } else if (cmd == "emu") {
        const int N = (int)next_double();
        const std::vector<double> v11 = next_vector((size_t)N * N), w_hat = next_vector(N);
        std::vector<double> alpha, Linv;
        const int rc = emulator_constants(v11.data(), w_hat.data(), N, alpha, Linv);
        done(rc);
        if (rc) return 0;
        put("alpha", alpha);
        put("Linv", Linv);
    } else if (cmd == "ext") {
        const int law = (int)next_double();
        const double Rv = next_double();
        std::vector<double> tab;
        const int rc = extinct_spline_table(law, Rv, tab);
        done(rc);
        if (!rc) put("tab", tab);
    } else if (cmd == "tw") {
        std::vector<double> tw;
        make_twiddles((int)next_double(), tw);
        done(SF_OK);
        put("tw", tw);
    } else if (cmd == "grid") {  // min_dv and the log-uniform test of a wavelength grid
        const int n = (int)next_double();
        const std::vector<double> w = next_vector(n);
        done(SF_OK);
        put("min_dv", {min_dv(w.data(), n)});
        put("loguniform", {is_loguniform(w.data(), n) ? 1.0 : 0.0});
    } else if (cmd == "band") {  // the band solver's shape (sf_band_shape.h) for every half-width 0 .. wmax, nrhs 1 .. nmax
        const int wmax = (int)next_double(), nmax = (int)next_double(), ncu = (int)next_double();
        done(SF_OK);
        std::vector<double> maxhw, shape, lds, workers, twist, carve, pays;
        for (int nrhs = 1; nrhs <= nmax; ++nrhs) maxhw.push_back(sf_band_max_halfwidth(nrhs));
        for (int w = 0; w <= wmax; ++w)
            for (int nrhs = 1; nrhs <= nmax; ++nrhs) {
                const int nbr = sfb_nbr(w), nrb = sfb_nrb(nrhs), nwaves = sfb_nwaves(nbr);
                for (int v : {(int)sfb_admit(w, nrhs), nbr, nrb, nwaves, sfb_loader_groups(nwaves)}) shape.push_back(v);
                const sfb_lds L = sfb_lds_layout(nbr, nrb);  // byte offsets of the regions, then the size
                for (int off : {L.Wb, L.RH, L.Fb2, L.G, L.pv, L.red, L.sync, L.ptab, L.reserve, L.doubles}) lds.push_back(8.0 * off);
                lds.push_back((double)L.bytes);
                for (int wave = 0; wave < 16; ++wave) {  // position and update pairs of every wave (-1: no such wave)
                    const int pos = wave < nwaves ? sfb_worker_pos(wave, nwaves) : -1;
                    workers.push_back(pos);
                    workers.push_back(pos < 0 ? -1 : sfb_worker_pairs(pos, nwaves - 1, nbr - 1 + nrb));
                }
                if (sfb_admit(w, nrhs) != SFB_WINDOW) continue;
                for (int batch = 1; batch <= 3; batch += 2) {  // carved from a real allocation of the counted size
                    const size_t count = sfb_twist_carve(nullptr, w, nrhs, batch).doubles;
                    const std::unique_ptr<double[]> buf(new double[count]);
                    const sfb_twist_work t = sfb_twist_carve(buf.get(), w, nrhs, batch);
                    for (int v : {w, nrhs, batch}) carve.push_back(v);
                    for (const double* p : {t.dumpM, t.dumpR, t.dumpG, t.dumpL, t.mband, t.mrhs, t.gadd, t.ladd})
                        carve.push_back((double)(p - buf.get()));
                    carve.push_back((double)t.doubles);
                    carve.push_back((double)count);
                }
            }
        for (int nbr = 3; nbr <= sfb_nbr(wmax); ++nbr)
            for (int nblk = 6 * nbr; nblk <= 300; ++nblk) {
                const sfb_twist t = sfb_twist_shape(nblk, nbr);
                for (int v : {nbr, nblk, t.nm, t.kend0, t.kend1, (int)sfb_twist_fits(nblk, nbr)}) twist.push_back(v);
            }
        for (int batch = 1; batch <= 1600; ++batch)  // cfg 2: 256 block columns, nbr = 10
            pays.push_back(sfb_twist_pays(256, 10, batch, ncu) ? 1.0 : 0.0);
        pays.push_back(sfb_twist_pays(6 * 10 - 1, 10, 1, ncu) ? 1.0 : 0.0);  // too few block columns for two halves
        put("consts", {(double)BB, (double)BS, (double)BLD, (double)SFB_PF, (double)SFB_PT, (double)SFB_LDS_MAX,
                       (double)SF_BAND_TILES_MAX_HALFWIDTH});
        put("maxhw", maxhw);
        put("shape", shape);
        put("lds", lds);
        put("workers", workers);
        put("twist", twist);
        put("carve", carve);
        put("pays", pays);
    } else {
        fprintf(stderr, "usage: hostmath_driver <lu|inv|emu|ext|tw|grid|band> < numbers\n");
        return 2;
    }
    return 0;
}
