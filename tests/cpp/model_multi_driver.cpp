// Test driver for the one-vs-all model files of the C++ host code (plssvm_sparse_fp22_amd/host/parameter.hpp;
// tests/test_model_multi.py):
//   model_multi_driver parse float|double <path>
//     "OK <K> <n> <d>", "LABELS l0 ...", "RHO r0 ...", "NRSV c0 ...", "KERNEL <k> <degree> <gamma> <coef0>", then one
//     line per support vector "a0 ... a(K-1) v0 ... v(d-1)" (%.17g); a binary model prints "BINARY <n> <d>";
//     or "ERROR <invalid_file_format|file_not_found|other>: <message>"
//   model_multi_driver rewrite float|double <path> <out>
//     parses the one-vs-all model and writes it again with the C++ writer's text (model_text_multi)
//   model_multi_driver labels float|double <path>
//     parses a LIBSVM data file with multiclass = true: "LABELS <class_labels ...>" and "SIGNS <labels ...>"
#include <cstdio>
#include <string>

#include "parameter.hpp"

template <typename T>
int run(const std::string &mode, const std::string &path, const char *out) {
    using namespace plssvm::mi355x;
    parameter<T> p;
    if (mode == "labels") {
        p.parse_train_file(path, false, true);
        std::printf("LABELS");
        for (const T v : p.class_labels) std::printf(" %.17g", (double) v);
        std::printf("\nSIGNS");
        for (const T v : p.labels) std::printf(" %.17g", (double) v);
        std::printf("\n");
        return 0;
    }
    try {
        p.parse_model_file(path);
    } catch (const invalid_file_format_exception &e) {
        std::printf("ERROR invalid_file_format: %s\n", e.what());
        return 0;
    } catch (const file_not_found_exception &e) {
        std::printf("ERROR file_not_found: %s\n", e.what());
        return 0;
    } catch (const std::exception &e) {
        std::printf("ERROR other: %s\n", e.what());
        return 0;
    }
    if (p.nr_class < 3) {
        std::printf("BINARY %lld %lld\n", (long long) p.num_data_points, (long long) p.num_features);
        return 0;
    }
    const std::size_t K = (std::size_t) p.nr_class;
    if (mode == "rewrite") {
        std::vector<int64_t> pc;
        std::vector<T> biases;
        for (std::size_t c = 0; c < K; ++c) {
            pc.insert(pc.end(), (std::size_t) p.nr_sv[c], (int64_t) c);
            biases.push_back(-p.rhos[c]);
        }
        const std::string text = p.model_text_multi(p.classes, pc, p.alphas, biases);
        std::FILE *fp = std::fopen(out, "w");
        if (!fp) return 3;
        std::fwrite(text.data(), 1, text.size(), fp);
        std::fclose(fp);
        return 0;
    }
    std::printf("OK %zu %lld %lld\nLABELS", K, (long long) p.num_data_points, (long long) p.num_features);
    for (const T v : p.classes) std::printf(" %.17g", (double) v);
    std::printf("\nRHO");
    for (const T v : p.rhos) std::printf(" %.17g", (double) v);
    std::printf("\nNRSV");
    for (const int64_t v : p.nr_sv) std::printf(" %lld", (long long) v);
    std::printf("\nKERNEL %s %d %.17g %.17g\n", kernel_name(p.kernel), p.degree, (double) p.gamma, (double) p.coef0);
    for (int64_t i = 0; i < p.num_data_points; ++i) {
        for (std::size_t c = 0; c < K; ++c) std::printf("%s%.17g", c ? " " : "", (double) p.alphas[c][(std::size_t) i]);
        for (int64_t f = 0; f < p.num_features; ++f) std::printf(" %.17g", (double) p.value(i, f));
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 4 || (std::string(argv[1]) == "rewrite" && argc != 5)) {
        std::fprintf(stderr, "usage: model_multi_driver parse|rewrite|labels float|double <path> [<out>]\n");
        return 2;
    }
    const std::string mode = argv[1], type = argv[2], path = argv[3];
    return type == "float" ? run<float>(mode, path, argc > 4 ? argv[4] : nullptr)
                           : run<double>(mode, path, argc > 4 ? argv[4] : nullptr);
}
