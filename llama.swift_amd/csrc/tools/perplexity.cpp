// perplexity -- the perplexity of a model file over a text, on top of llamahip_perplexity:
//   perplexity MODEL (--file PATH | --prompt TEXT) [--ctx 512] [--threads 8] [--score-from N] [--chunk N] [--fast-prefill]
// The text is tokenized with BOS and cut into windows of --ctx tokens (the tail that does not fill one is unused); the second half of
// every window is scored (--score-from N: from row N; 0 = every row).  Prints the running perplexity after each window on one line,
// then `ppl <%.17g> n_scored <n> windows <k> ms <t>`.  LLAMAHIP_DEVICES splits the layers over devices as for every other caller.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/llamahip.h"

static int usage() {
    fprintf(stderr, "usage: perplexity MODEL (--file PATH | --prompt TEXT) [--ctx 512] [--threads 8] [--score-from N] [--chunk N] [--fast-prefill]\n");
    return 2;
}

int main(int argc, char **argv) {
    if (argc < 2) return usage();
    std::string text;
    bool have_text = false, fast = false;
    int ctx = 512, threads = 8, score_from = -1, chunk = 0;
    for (int i = 2; i < argc; i++) {
        const std::string k = argv[i];
        const bool more = i + 1 < argc;
        if (k == "--file" && more) {
            std::ifstream f(argv[++i], std::ios::binary);
            if (!f) { fprintf(stderr, "perplexity: cannot read '%s'\n", argv[i]); return 1; }
            std::stringstream ss;
            ss << f.rdbuf();
            text = ss.str();
            have_text = true;
        } else if (k == "--prompt" && more) { text = argv[++i]; have_text = true; }
        else if (k == "--ctx" && more) ctx = atoi(argv[++i]);
        else if (k == "--threads" && more) threads = atoi(argv[++i]);
        else if (k == "--score-from" && more) score_from = atoi(argv[++i]);
        else if (k == "--chunk" && more) chunk = atoi(argv[++i]);
        else if (k == "--fast-prefill") fast = true;
        else return usage();
    }
    if (!have_text || ctx < 2) return usage();

    char err[512] = { 0 };
    llamahip_opts opts;
    memset(&opts, 0, sizeof(opts));
    opts.struct_size = (int32_t) sizeof(opts);
    opts.device = -1;
    opts.layer_end = -1;
    opts.flags = fast ? LLAMAHIP_FLAG_FAST_PREFILL : 0;
    llamahip_model *m = nullptr;
    if (llamahip_model_load(argv[1], ctx, &opts, &m, err, sizeof(err)) != 0) {
        fprintf(stderr, "perplexity: failed to load '%s': %s\n", argv[1], err);
        return 1;
    }
    std::vector<int32_t> toks(text.size() + 2);
    int32_t n = llamahip_tokenize(m, text.c_str(), 1, toks.data(), (int32_t) toks.size());
    if (n > (int32_t) toks.size()) { toks.resize(n); n = llamahip_tokenize(m, text.c_str(), 1, toks.data(), n); }
    toks.resize(n > 0 ? (size_t) n : 0);
    const int n_win = ctx > 0 ? (int) toks.size() / ctx : 0;
    fprintf(stderr, "perplexity: %zu tokens, %d windows of %d\n", toks.size(), n_win, ctx);

    std::vector<double> running(n_win > 0 ? n_win : 1);
    double nll = 0.0;
    int64_t n_scored = 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = llamahip_perplexity(m, threads, toks.data(), (int32_t) toks.size(), ctx, score_from, chunk, &nll, &n_scored, running.data(), err, sizeof(err));
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != 0) {
        fprintf(stderr, "perplexity: %s\n", err);
        llamahip_model_free(m);
        return 1;
    }
    for (int k = 0; k < n_win; k++) printf("[%d]%.4f%s", k + 1, running[k], k + 1 < n_win ? "," : "\n");
    printf("ppl %.17g n_scored %lld windows %d ms %.3f\n", exp(nll / (double) n_scored), (long long) n_scored, n_win, ms);
    llamahip_model_free(m);
    return 0;
}
