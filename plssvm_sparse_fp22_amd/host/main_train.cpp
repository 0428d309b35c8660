// plssvm-train for the MI355X backend: same flags, defaults and output as the reference executable
// (src/main_train.cpp:27-91, src/plssvm/parameter_train.cpp:38-142), training through
// plssvm::mi355x::csvm<T> (host/csvm.hpp) on libplssvm_mi355x.so.
//
// Additions (not in the reference): --sparse keeps LIBSVM input as CSR (the reference densifies),
// --max_iter overrides the CG limit (default: num_features, csvm.cpp:256), --single trains in fp32
// (the reference selects that at compile time, main_train.cpp:21-25), --device picks the GPU, --multiclass trains
// one-vs-all over the file's distinct labels (three or more) and writes the one-vs-all model file, --class_weights
// L1:W1,L2:W2 trains the points of label Li at cost C * Wi (LIBSVM's -wi; with --multiclass: the positives of class Li),
// -v n runs n-fold cross-validation instead of training (LIBSVM's -v: no model file; stratified folds without random
// numbers, csvm<T>::stratified_folds) and --cv_costs c1,c2,... does so at every listed cost in the same pass.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "cli.hpp"
#include "csvm.hpp"

namespace {

const char *kHelp =
    "LS-SVM with multiple (GPU-)backends\n"
    "Usage:\n"
    "  plssvm-train [OPTION...] training_set_file [model_file]\n\n"
    "  -t, --kernel_type arg      set type of kernel function.\n"
    "                                  0 -- linear: u'*v\n"
    "                                  1 -- polynomial: (gamma*u'*v + coef0)^degree\n"
    "                                  2 -- radial basis function: exp(-gamma*|u-v|^2)\n"
    "                                  4 -- laplacian: exp(-gamma*|u-v|_1), dense input only (default: 0)\n"
    "  -d, --degree arg           set degree in kernel function (default: 3)\n"
    "  -g, --gamma arg            set gamma in kernel function (default: 1 / num_features)\n"
    "  -r, --coef0 arg            set coef0 in kernel function (default: 0)\n"
    "  -c, --cost arg             set the parameter C (default: 1)\n"
    "  -e, --epsilon arg          set the tolerance of termination criterion (default: 0.001)\n"
    "  -b, --backend arg          choose the backend: automatic|hip (default: automatic)\n"
    "  -p, --target_platform arg  choose the target platform: automatic|gpu_amd (default: automatic)\n"
    "  -q, --quiet                quiet mode (no outputs)\n"
    "  -h, --help                 print this helper message\n"
    "      --sparse               keep the data as CSR on the device (MI355X backend addition)\n"
    "      --max_iter arg         maximum CG iterations (default: num_features)\n"
    "      --single               train in single precision (float)\n"
    "      --device arg           train on this one HIP device (default: every visible device)\n"
    "      --devices arg          comma-separated device list, one rank per entry (a device listed twice:\n"
    "                             in-process host exchange instead of RCCL)\n"
    "      --multiclass           one-vs-all over the file's distinct labels (three or more classes)\n"
    "      --class_weights arg    L1:W1,L2:W2,...: train the points of label Li at cost C * Wi, all others at C\n"
    "                             (with --multiclass: the points of class Li in class Li's own problem)\n"
    "  -v, --cross_validation arg n-fold cross validation mode: prints the accuracy, writes no model (one device)\n"
    "      --cv_costs arg         c1,c2,...: with -v, the accuracy at each of these costs and the best one\n";

// "L1:W1,L2:W2" -> {label: weight}; false (with the reason in why) for a malformed list or a weight that is not > 0
template <typename T>
bool parse_class_weights(const std::string &list, std::map<T, T> &out, std::string &why) {
    out.clear();
    for (size_t a = 0; a <= list.size();) {
        const size_t b = std::min(list.find(',', a), list.size());
        const std::string item = list.substr(a, b - a);
        const size_t colon = item.find(':');
        if (colon == std::string::npos || colon == 0 || colon + 1 >= item.size()) {
            why = "'" + item + "' is not of the form label:weight";
            return false;
        }
        char *e1 = nullptr, *e2 = nullptr;
        const std::string ls = item.substr(0, colon), ws = item.substr(colon + 1);
        const double l = std::strtod(ls.c_str(), &e1), w = std::strtod(ws.c_str(), &e2);
        if (*e1 != '\0' || *e2 != '\0' || !std::isfinite(l)) {
            why = "'" + item + "' is not of the form label:weight";
            return false;
        }
        if (!(w > 0) || !std::isfinite(w) || !((T) w > T(0)) || !std::isfinite((T) w)) {
            why = "the weight of label " + ls + " must be a finite number > 0, not " + ws;
            return false;
        }
        if (!out.emplace((T) l, (T) w).second) {
            why = "the label " + ls + " is listed twice";
            return false;
        }
        a = b + 1;
    }
    return true;
}

template <typename T>
int train(const cli &c) {
    using namespace plssvm::mi355x;
    parameter<T> params;
    if (c.opt.count("kernel_type")) params.kernel = parse_kernel(c.opt.at("kernel_type"));
    if (c.opt.count("degree")) params.degree = std::stoi(c.opt.at("degree"));
    if (c.opt.count("gamma")) {
        params.gamma = to_real<T>(c.opt.at("gamma"));
        if (params.gamma == T(0)) {
            std::fprintf(stderr, "gamma = 0.0 is not allowed, it doesnt make any sense!\n");
            std::printf("%s", kHelp);
            return EXIT_FAILURE;
        }
    }
    if (c.opt.count("coef0")) params.coef0 = to_real<T>(c.opt.at("coef0"));
    if (c.opt.count("cost")) params.cost = to_real<T>(c.opt.at("cost"));
    if (c.opt.count("epsilon")) params.epsilon = to_real<T>(c.opt.at("epsilon"));
    const std::string backend = c.opt.count("backend") ? c.opt.at("backend") : "automatic";
    if (backend != "automatic" && backend != "hip" && backend != "mi355x")
        throw std::invalid_argument("Unavailable backend: '" + backend + "' (this build provides hip = MI355X)");
    const std::string target = c.opt.count("target_platform") ? c.opt.at("target_platform") : "automatic";
    if (target != "automatic" && target != "gpu_amd")
        throw std::invalid_argument("Invalid target platform '" + target + "' for the HIP backend!");
    params.print_info = !c.opt.count("quiet");
    if (c.pos.empty()) {
        std::fprintf(stderr, "Error missing input file!");
        std::printf("%s", kHelp);
        return EXIT_FAILURE;
    }
    params.input_filename = c.pos[0];
    if (c.pos.size() > 1) params.model_filename = c.pos[1];
    if (params.kernel == kernel_type::laplacian && c.opt.count("sparse") > 0) {  // before the file is read or a GPU touched
        std::fprintf(stderr, "The laplacian kernel takes dense input: it cannot be combined with --sparse!\n");
        return EXIT_FAILURE;
    }
    // cross-validation: what the options alone decide, before the file is read or a GPU touched
    const bool cv = c.opt.count("cross_validation") > 0;
    long long nfold = 0;
    std::vector<T> cv_costs;
    if (c.opt.count("cv_costs") && !cv) {
        std::fprintf(stderr, "--cv_costs needs -v (the number of folds)!\n");
        return EXIT_FAILURE;
    }
    if (cv) {
        char *end = nullptr;
        const std::string &vs = c.opt.at("cross_validation");
        nfold = std::strtoll(vs.c_str(), &end, 10);
        if (vs.empty() || *end != '\0' || nfold < 2) {
            std::fprintf(stderr, "-v: n-fold cross validation needs n >= 2, not '%s'!\n", vs.c_str());
            return EXIT_FAILURE;
        }
        if (c.opt.count("multiclass")) {
            std::fprintf(stderr, "-v cross-validates the binary problem: it cannot be combined with --multiclass!\n");
            return EXIT_FAILURE;
        }
        if (c.opt.count("devices") && c.opt.at("devices").find(',') != std::string::npos) {
            std::fprintf(stderr, "-v runs on one device: --devices lists more than one!\n");
            return EXIT_FAILURE;
        }
        if (c.opt.count("cv_costs")) {
            const std::string &l = c.opt.at("cv_costs");
            for (size_t a = 0; a <= l.size();) {
                const size_t b = std::min(l.find(',', a), l.size());
                const std::string item = l.substr(a, b - a);
                char *e = nullptr;
                const double v = std::strtod(item.c_str(), &e);
                if (item.empty() || *e != '\0' || !(v > 0) || !std::isfinite(v) || !((T) v > T(0)) || !std::isfinite((T) v)) {
                    std::fprintf(stderr, "--cv_costs: '%s' is not a finite number > 0!\n", item.c_str());
                    return EXIT_FAILURE;
                }
                cv_costs.push_back((T) v);
                a = b + 1;
            }
        }
    }
    std::map<T, T> weights;
    if (c.opt.count("class_weights")) {  // syntax and signs: before the file is read or a GPU touched
        std::string why;
        if (!parse_class_weights<T>(c.opt.at("class_weights"), weights, why)) {
            std::fprintf(stderr, "--class_weights: %s!\n", why.c_str());
            return EXIT_FAILURE;
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    const bool multiclass = c.opt.count("multiclass") > 0;
    // class weights name the labels as the file writes them: keep those values beside their signs
    params.parse_train_file(c.pos[0], c.opt.count("sparse") > 0, multiclass || !weights.empty());
    for (const auto &kv : weights)
        if (std::find(params.class_labels.begin(), params.class_labels.end(), kv.first) == params.class_labels.end()) {
            std::fprintf(stderr, "--class_weights: the label %s does not occur in '%s'!\n", csvm<T>::shortest(kv.first).c_str(),
                         c.pos[0].c_str());
            return EXIT_FAILURE;
        }
    if (c.pos.size() > 1) params.model_filename = c.pos[1];
    if (cv && nfold > (long long) params.num_data_points) {
        std::fprintf(stderr, "-v: %lld folds are more than the %lld data points of '%s'!\n", nfold, (long long) params.num_data_points,
                     c.pos[0].c_str());
        return EXIT_FAILURE;
    }
    if (multiclass) {
        std::vector<T> distinct = params.class_labels;
        std::sort(distinct.begin(), distinct.end());
        distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
        if (distinct.size() < 3) {
            std::fprintf(stderr, "--multiclass needs at least 3 distinct labels, but %zu were given! Train without it for two classes.\n",
                         distinct.size());
            return EXIT_FAILURE;
        }
    }
    if (params.print_info) {
        std::printf("Read %lld data points with %lld features in %lldms using the libsvm parser from file '%s'.\n\n",
                    (long long) params.num_data_points, (long long) params.num_features,
                    (long long) std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count(),
                    params.input_filename.c_str());
        std::printf("task: training\nkernel type: %s -> ", kernel_name(params.kernel));
        switch (params.kernel) {
            case kernel_type::linear: std::printf("u'*v\n"); break;
            case kernel_type::polynomial:
                std::printf("(gamma*u'*v + coef0)^degree\ngamma: %s\ncoef0: %s\ndegree: %d\n",
                            csvm<T>::shortest(params.gamma).c_str(), csvm<T>::shortest(params.coef0).c_str(), params.degree);
                break;
            case kernel_type::laplacian: std::printf("exp(-gamma*|u-v|_1)\ngamma: %s\n", csvm<T>::shortest(params.gamma).c_str()); break;
            default: std::printf("exp(-gamma*|u-v|^2)\ngamma: %s\n", csvm<T>::shortest(params.gamma).c_str()); break;
        }
        std::printf("cost: %s\nepsilon: %s\ninput file (data set): '%s'\noutput file (model): '%s'\n\n",
                    csvm<T>::shortest(params.cost).c_str(), csvm<T>::shortest(params.epsilon).c_str(),
                    params.input_filename.c_str(), params.model_filename.c_str());
        std::printf("Using HIP (MI355X, gfx950) as backend.\n");
    }
    // hip::csvm<T>(params) takes every visible device (csvm.hip.cpp:53-55): here one rank of a row-block group per
    // device; --device keeps one, --devices lists them
    std::vector<int> devs;
    if (c.opt.count("devices")) {
        const std::string &l = c.opt.at("devices");
        for (size_t a = 0; a <= l.size();) {
            const size_t b = std::min(l.find(',', a), l.size());
            devs.push_back(std::stoi(l.substr(a, b - a)));
            a = b + 1;
        }
    } else if (c.opt.count("device")) {
        devs.push_back(std::stoi(c.opt.at("device")));
    } else if (cv) {
        devs.push_back(0);
    } else {
        devs = csvm<T>::all_devices(params);
    }
    csvm<T> svm(params, devs);
    svm.set_class_weights(weights);
    if (params.print_info) {
        std::printf("Found %d HIP device(s):\n", svm.num_devices());
        for (const int d : svm.devices()) std::printf("  [%d, gfx950]\n", d);
        std::printf("\n");
    }
    if (cv) {
        // LIBSVM's -v: the accuracy on the held-out folds, no model file
        const std::size_t imax = c.opt.count("max_iter") ? (std::size_t) std::stoll(c.opt.at("max_iter")) : (std::size_t) params.num_features;
        const std::vector<double> acc = svm.cross_validate((std::size_t) nfold, cv_costs, imax);
        if (cv_costs.empty()) {
            std::printf("Cross Validation Accuracy = %g%%\n", 100 * acc[0]);
        } else {
            size_t best = 0;
            for (size_t k = 0; k < acc.size(); ++k) {
                std::printf("C = %s: Cross Validation Accuracy = %g%%\n", csvm<T>::shortest(cv_costs[k]).c_str(), 100 * acc[k]);
                // a tie goes to the smaller cost
                if (acc[k] > acc[best] || (acc[k] == acc[best] && cv_costs[k] < cv_costs[best])) best = k;
            }
            std::printf("Best C = %s (Cross Validation Accuracy = %g%%)\n", csvm<T>::shortest(cv_costs[best]).c_str(), 100 * acc[best]);
        }
        return EXIT_SUCCESS;
    }
    // learn() prints the reference's setup line, one line per CG iteration and the solve summary
    // (csvm.cpp:226-266, OpenMP/csvm.cpp:115-117,161-166)
    if (multiclass) {
        // one summary line per class instead of the per-iteration lines (the multi entry points report no progress)
        if (c.opt.count("max_iter")) svm.learn_multi((std::size_t) std::stoll(c.opt.at("max_iter")));
        else svm.learn_multi();
        if (params.print_info) {
            for (size_t k = 0; k < svm.classes().size(); ++k) {
                const std::vector<double> &tr = svm.residual_traces()[k];
                std::printf("Class %s: finished after %lld iterations with a residuum of %s (target: %s).\n",
                            csvm<T>::shortest(svm.classes()[k]).c_str(), (long long) svm.iterations_multi()[k],
                            csvm<T>::shortest((T) tr.back()).c_str(),
                            csvm<T>::shortest(params.epsilon * params.epsilon * (T) tr.front()).c_str());
            }
        }
    } else if (c.opt.count("max_iter")) {
        svm.learn((std::size_t) std::stoll(c.opt.at("max_iter")));
    } else {
        svm.learn();
    }
    svm.write_model(params.model_filename);
    if (params.print_info) std::printf("Wrote model file ('%s').\n", params.model_filename.c_str());
    return EXIT_SUCCESS;
}

}  // namespace

int main(int argc, char **argv) {
    try {
        const cli c = parse_cli(argc, argv, { { "t", "kernel_type" }, { "d", "degree" }, { "g", "gamma" }, { "r", "coef0" },
                                              { "c", "cost" }, { "e", "epsilon" }, { "b", "backend" },
                                              { "p", "target_platform" }, { "q", "quiet" }, { "h", "help" },
                                              { "v", "cross_validation" } },
                                { "quiet", "help", "sparse", "single", "multiclass" });
        if (c.opt.count("help")) {
            std::printf("%s", kHelp);
            return EXIT_SUCCESS;
        }
        return c.opt.count("single") ? train<float>(c) : train<double>(c);
    } catch (const std::exception &e) {
        std::cerr << e.what() << std::endl;
        return EXIT_FAILURE;
    }
}
