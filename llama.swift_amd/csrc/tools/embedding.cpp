// embedding -- the embeddings of the texts of a file, one text per line, on top of llamahip_text_embedding_multi:
//   embedding MODEL (--file PATH | --prompt TEXT) [--pool last|mean] [--no-normalize] [--cosine] [--ctx 512] [--threads 8] [--chunk N] [--batch 16]
// Every line is tokenized with BOS (an empty line is skipped; a line longer than --ctx tokens is cut there) and up to --batch (at most 16)
// texts are evaluated per weight pass, each on a KV slot of its own.  Prints one line per text: `n_embd` numbers (%.9g), or with --cosine the
// similarity matrix -- row i: dot(e_i, e_j) / (|e_i| |e_j|) for every j, summed in double (%.6f).  Then, on stderr, `texts <n> passes <k> ms <t>`.
// LLAMAHIP_DEVICES splits the layers over devices as for every other caller.
#include <algorithm>
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
    fprintf(stderr, "usage: embedding MODEL (--file PATH | --prompt TEXT) [--pool last|mean] [--no-normalize] [--cosine] [--ctx 512] [--threads 8] [--chunk N] [--batch 16]\n");
    return 2;
}

int main(int argc, char **argv) {
    if (argc < 2) return usage();
    std::string text;
    bool have_text = false, cosine = false;
    int ctx = 512, threads = 8, chunk = 0, batch = LLAMAHIP_POOL_MAX_SEGS, pool = LLAMAHIP_POOL_MEAN, normalize = 1;
    for (int i = 2; i < argc; i++) {
        const std::string k = argv[i];
        const bool more = i + 1 < argc;
        if (k == "--file" && more) {
            std::ifstream f(argv[++i], std::ios::binary);
            if (!f) { fprintf(stderr, "embedding: cannot read '%s'\n", argv[i]); return 1; }
            std::stringstream ss;
            ss << f.rdbuf();
            text = ss.str();
            have_text = true;
        } else if (k == "--prompt" && more) { text = argv[++i]; have_text = true; }
        else if (k == "--pool" && more) {
            const std::string p = argv[++i];
            if (p != "last" && p != "mean") return usage();
            pool = p == "last" ? LLAMAHIP_POOL_LAST : LLAMAHIP_POOL_MEAN;
        }
        else if (k == "--no-normalize") normalize = 0;
        else if (k == "--cosine") cosine = true;
        else if (k == "--ctx" && more) ctx = atoi(argv[++i]);
        else if (k == "--threads" && more) threads = atoi(argv[++i]);
        else if (k == "--chunk" && more) chunk = atoi(argv[++i]);
        else if (k == "--batch" && more) batch = atoi(argv[++i]);
        else return usage();
    }
    if (!have_text || ctx < 1 || batch < 1 || batch > LLAMAHIP_POOL_MAX_SEGS) return usage();

    char err[512] = { 0 };
    llamahip_opts opts;
    memset(&opts, 0, sizeof(opts));
    opts.struct_size = (int32_t) sizeof(opts);
    opts.device = -1;
    opts.layer_end = -1;
    opts.n_seq = batch;
    llamahip_model *m = nullptr;
    if (llamahip_model_load(argv[1], ctx, &opts, &m, err, sizeof(err)) != 0) {
        fprintf(stderr, "embedding: failed to load '%s': %s\n", argv[1], err);
        return 1;
    }
    // one text per line
    std::vector<std::vector<int32_t>> texts;
    std::stringstream lines(text);
    for (std::string line; std::getline(lines, line);) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        std::vector<int32_t> toks(line.size() + 2);
        int32_t n = llamahip_tokenize(m, line.c_str(), 1, toks.data(), (int32_t) toks.size());
        if (n > (int32_t) toks.size()) { toks.resize(n); n = llamahip_tokenize(m, line.c_str(), 1, toks.data(), n); }
        toks.resize(n > 0 ? (size_t) std::min(n, ctx) : 0);
        if (!toks.empty()) texts.push_back(toks);
    }
    const size_t T = texts.size(), d = (size_t) llamahip_n_embd(m);
    std::vector<float> emb(std::max(T, (size_t) 1) * d);
    int passes = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t b0 = 0; b0 < T;) {
        // as many of the next texts as fit a pass: at most `batch`, at most LLAMAHIP_EVAL_MULTI_MAX_ROWS rows
        std::vector<int32_t> slots, past, flat, nt;
        size_t b1 = b0;
        while (b1 < T && (int) (b1 - b0) < batch && flat.size() + texts[b1].size() <= LLAMAHIP_EVAL_MULTI_MAX_ROWS) {
            slots.push_back((int32_t) (b1 - b0)); past.push_back(0); nt.push_back((int32_t) texts[b1].size());
            flat.insert(flat.end(), texts[b1].begin(), texts[b1].end());
            b1++;
        }
        if (b1 == b0) { fprintf(stderr, "embedding: text %zu has more than %d tokens\n", b0, LLAMAHIP_EVAL_MULTI_MAX_ROWS); llamahip_model_free(m); return 1; }
        const int rc = llamahip_text_embedding_multi(m, threads, (int32_t) slots.size(), slots.data(), past.data(), flat.data(), nt.data(), chunk, pool, normalize,
                                                     emb.data() + b0 * d, nullptr, err, sizeof(err));
        if (rc != 0) { fprintf(stderr, "embedding: %s\n", err); llamahip_model_free(m); return 1; }
        passes++;
        b0 = b1;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (cosine) {
        std::vector<double> len(T);
        for (size_t i = 0; i < T; i++) { double s = 0.0; for (size_t c = 0; c < d; c++) s += (double) emb[i * d + c] * (double) emb[i * d + c]; len[i] = sqrt(s); }
        for (size_t i = 0; i < T; i++)
            for (size_t j = 0; j < T; j++) {
                double s = 0.0;
                for (size_t c = 0; c < d; c++) s += (double) emb[i * d + c] * (double) emb[j * d + c];
                const double den = len[i] * len[j];
                printf("%.6f%s", den > 0.0 ? s / den : 0.0, j + 1 < T ? " " : "\n");
            }
    } else {
        for (size_t i = 0; i < T; i++)
            for (size_t c = 0; c < d; c++) printf("%.9g%s", emb[i * d + c], c + 1 < d ? " " : "\n");
    }
    fprintf(stderr, "texts %zu passes %d ms %.3f\n", T, passes, ms);
    llamahip_model_free(m);
    return 0;
}
