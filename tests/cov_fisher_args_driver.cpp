// Stand-alone driver for the host side of sf_fisher_cov_batch -- the argument checks and the workspace layout (carve_applied
// with AW_FISHER_COV) -- under AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU.  Nothing here touches a device: the
// context is a host-side sf_ctx with the sizes of an order and no device buffers, which is all that the size query and the
// refusals look at.  Build the library's host code with the sanitizers and link this program against it:
//     make -C starfish_amd/csrc TAG=san CXX=clang++ EXTRA="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
//     hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//           -I starfish_amd/csrc -I include tests/cov_fisher_args_driver.cpp -L starfish_amd -lstarfish_amd_san \
//           -Wl,-rpath,$PWD/starfish_amd -o cov_fisher_args_driver
// Prints one line per check and "ok"; exit status 1 on the first mismatch.
#include <stdio.h>
#include <string.h>

#include "../include/starfish_amd.h"
#include "sf_ctx.h"

static int fails = 0;
static void expect(bool ok, const char* what) {
    printf("%s %s\n", ok ? "pass" : "FAIL", what);
    if (!ok) ++fails;
}
static bool refused(int rc, const char* word) {
    const char* msg = sf_last_error();
    return rc == SF_EINVAL && strncmp(msg, "sf_fisher_cov_batch:", 20) == 0 && strstr(msg, word);
}

int main() {
    double* fake = (double*)0x10000;  // (never dereferenced: every call below returns before it enqueues anything)
    sf_model_desc md;
    memset(&md, 0, sizeof md);
    md.has_global = 1, md.n_local = 1, md.has_log_scale = 1;
    sf_model_desc none = md;
    none.has_global = 0, none.n_local = 0;
    const size_t big = (size_t)1 << 40;
    // refusals before the context is looked at
    expect(refused(sf_fisher_cov_batch(nullptr, &md, 0, fake, nullptr, fake, 25, nullptr, fake, big, nullptr), "B=0"), "B = 0");
    expect(refused(sf_fisher_cov_batch(nullptr, &md, 65536, fake, nullptr, fake, 25, nullptr, fake, big, nullptr), "B=65536"), "B = 65536");
    expect(refused(sf_fisher_cov_batch(nullptr, &md, 3, nullptr, nullptr, fake, 25, nullptr, fake, big, nullptr), "required"), "null d_params");
    expect(refused(sf_fisher_cov_batch(nullptr, &md, 3, fake, nullptr, nullptr, 25, nullptr, fake, big, nullptr), "required"), "null d_fisher");
    expect(refused(sf_fisher_cov_batch(nullptr, &none, 3, fake, nullptr, fake, 25, nullptr, fake, big, nullptr), "nothing to differentiate"),
           "no structured kernel");
    expect(refused(sf_fisher_cov_batch(nullptr, &md, 3, fake, nullptr, fake, 24, nullptr, fake, big, nullptr), "fisher_stride=24"),
           "fisher_stride < s^2");
    expect(sf_fisher_cov_batch(nullptr, &md, 3, fake, nullptr, fake, 25, nullptr, fake, big, nullptr) == SF_EINVAL &&
               strcmp(sf_last_error(), "bad context / model descriptor") == 0,
           "good counts, no context");
    expect(sf_fisher_cov_workspace_bytes(nullptr, &md, 3) == 0 && sf_fisher_cov_workspace_bytes(nullptr, nullptr, 3) == 0,
           "size query without a context");
    // the layout on a host-side context with an order's sizes: n = 180 (npad 192) and n = 4000 (npad 4032)
    const int orders[2][2] = {{180, 192}, {4000, 4032}};
    for (const auto& nn : orders) {
        sf_ctx c;
        c.n = nn[0], c.npad = nn[1], c.lda = nn[1] + 16, c.m = 4, c.mpad = 16, c.M = 40, c.P = 3, c.nf = 512, c.rows = 5;
        const size_t ld = (size_t)(c.n + 63) / 64 * 64;
        expect(sf_fisher_cov_workspace_bytes(&c, &md, 0) == 0 && sf_fisher_cov_workspace_bytes(&c, &none, 3) == 0, "size 0 for refusals");
        size_t last = 0;
        for (int B : {1, 3, 64}) {
            const size_t grad = sf_loglike_grad_workspace_bytes(&c, &md, B), fisher = sf_fisher_cov_workspace_bytes(&c, &md, B);
            expect(grad > 0 && fisher == grad + 2 * sizeof(double) * (size_t)B * ld * ld, "the gradient's workspace plus W and one T_j");
            expect(fisher > last, "grows with B");
            last = fisher;
            sf_model_desc two = md;
            two.has_global = 0, two.n_local = 2;
            expect(sf_fisher_cov_workspace_bytes(&c, &two, B) - sf_loglike_grad_workspace_bytes(&c, &two, B) == fisher - grad,
                   "the quadratic part does not depend on the slots");
        }
        // a workspace a byte short is refused or, without a device, the call stops where it selects one: never a success
        const size_t need = sf_fisher_cov_workspace_bytes(&c, &md, 3);
        expect(sf_fisher_cov_batch(&c, &md, 3, fake, nullptr, fake, 25, nullptr, fake, need - 1, nullptr) != SF_OK, "a byte short");
    }
    printf(fails ? "FAILED %d\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
