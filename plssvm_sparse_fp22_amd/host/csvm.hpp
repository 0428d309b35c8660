// plssvm::mi355x::csvm<T> — the reference's plssvm::csvm<T> / hip::csvm<T> surface over the C ABI
// (include/plssvm_mi355x.h). Host-only C++17; all compute runs in libplssvm_mi355x.so on the GPU.
//
// Derives from csvm_interface<T> (csvm_interface.hpp: the reference's abstract plssvm::csvm<T>, restated:
// same pure virtuals, state, constructor checks and learn()) and implements its five pure virtuals on the
// C ABI — exactly what a maintainer's hip::csvm<T> replacement does. The hooks
// mock_hip_csvm exposes (tests/backends/HIP/mock_hip_csvm.hpp:24-51) are public here; write_model()
// writes the LIBSVM model format of csvm.cpp:60-204.
#pragma once

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/plssvm_mi355x.h"
#include "../../include/plssvm_mi355x_group.hpp"
#include "csvm_interface.hpp"
#include "parameter.hpp"

namespace plssvm::mi355x {

struct backend_exception : std::runtime_error {  // plssvm::hip::backend_exception
    int code;
    backend_exception(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

template <typename T>
class csvm : public csvm_interface<T> {
    using base = csvm_interface<T>;

  public:
    using real_type = T;
    using base::learn;  // learn() (imax = num_features) and learn(imax)

    // hip::csvm<T>(params) (src/plssvm/backends/HIP/csvm.hip.cpp:38-81): every visible GPU of the node, one host
    // thread and one context per GPU in a row-block group (RCCL), at most one GPU per row of the m = N - 1 rows
    explicit csvm(const parameter<T> &params) : csvm(params, all_devices(params)) {}
    // one GPU (plssvm-train --device N)
    csvm(const parameter<T> &params, int device) : csvm(params, std::vector<int>{ device }) {}
    // an explicit device list; a device listed twice forms the group over the in-process host exchange
    // (device_group: two contexts on one GPU, which RCCL refuses — the multi-rank path's test transport)
    csvm(const parameter<T> &params, const std::vector<int> &devices,
         device_group::transport tr = device_group::transport::automatic) :
        base(params) {
        try {
            grp_ = std::make_unique<device_group>(devices, (int) sizeof(T), (int) this->kernel_, this->degree_,
                                                  (double) this->gamma_, (double) this->coef0_, (double) this->cost_, tr);
        } catch (const group_error &e) {
            throw backend_exception(e.code, e.what());
        }
    }

    // the visible GPUs the default constructor takes: min(#GPUs, m), like the reference's min(#GPUs, #features)
    // feature split (csvm.hip.cpp:53-55), here over rows
    static std::vector<int> all_devices(const parameter<T> &params) {
        const int n = plssvm_mi_device_count();
        if (n <= 0) throw backend_exception(PLSSVM_MI_ERR_NODEV, "HIP backend selected but no HIP devices were found!");
        const int64_t m = std::max<int64_t>(params.num_data_points - 1, 1);
        std::vector<int> d((size_t) std::min<int64_t>(n, m));
        for (size_t k = 0; k < d.size(); ++k) d[k] = (int) k;
        return d;
    }
    int num_devices() const { return grp_->size(); }
    const std::vector<int> &devices() const { return grp_->devices(); }

    // one process per GPU instead (MPI / torch launchers): a one-device csvm joins a row-block group before setup
    // (rank 0 creates the id)
    void join_group(int rank, int world, const void *unique_id) {
        if (grp_->size() != 1) throw exception{ "join_group needs a one-device csvm" };
        on_all([&](int, plssvm_mi_ctx *c) { return plssvm_mi_comm_init(c, rank, world, unique_id); });
    }

    // ---- the reference's pure virtuals (csvm.hpp:188-214), public here like mock_hip_csvm's hooks ----
    // every call runs on all ranks at once (their collectives meet inside the library); outputs come from rank 0
    void setup_data_on_device() override {
        const auto &p = this->params_;
        on_all([&](int, plssvm_mi_ctx *c) {
            if (p.sparse) {
                const bool f22 = !p.val22.empty() && sizeof(T) == 4;  // packed FP22 input stays packed
                return plssvm_mi_setup_csr(c, p.rowptr.data(), p.col.data(), f22 ? (const void *) p.val22.data() : p.val.data(),
                                           f22 ? PLSSVM_MI_VAL_FP22 : PLSSVM_MI_VAL_REAL, p.num_data_points, p.num_features);
            }
            return plssvm_mi_setup_dense(c, p.dense.data(), p.num_data_points, p.num_features);
        });
        on_device_ = true;
    }
    [[nodiscard]] std::vector<T> generate_q() override {
        const size_t len = std::max<std::size_t>(this->num_data_points_ - 1, 1);
        std::vector<T> q(len);
        auto sc = scratch(len);
        on_all([&](int r, plssvm_mi_ctx *c) {
            double qa = 0;
            return plssvm_mi_generate_q(c, r == 0 ? q.data() : sc[(size_t) r].data(), &qa);
        });
        q.resize(this->num_data_points_ - 1);
        return q;
    }
    // with print_info, the reference's per-iteration lines (OpenMP/csvm.cpp:115-117,161-166): the residual
    // before each iteration and the stop target, streamed per polled batch of device iterations; the
    // "Done in" time of an iteration is its batch's wall time / iterations (the device runs a batch
    // without host round trips), truncated to ms like the reference's duration_cast
    std::vector<T> solver_CG(const std::vector<T> &b, std::size_t imax, T eps, const std::vector<T> &q) override {
        const size_t len = std::max<std::size_t>(b.size(), 1);
        std::vector<T> x(len);
        auto sc = scratch(len);
        std::vector<std::vector<double>> tr((size_t) grp_->size(), std::vector<double>(imax + 1, 0.0));
        std::vector<int64_t> its((size_t) grp_->size(), 0);
        progress_state ps{ (int64_t) imax, 0.0, 0.0, 0 };
        on_all([&](int r, plssvm_mi_ctx *c) {
            int rc = plssvm_mi_set_qa_cost(c, (double) this->QA_cost_);  // learn() computed it on the host
            if (rc != PLSSVM_MI_OK) return rc;
            if (this->print_info_ && r == 0) {
                rc = plssvm_mi_set_progress(c, &csvm::print_progress, &ps);
                if (rc != PLSSVM_MI_OK) return rc;
            }
            rc = plssvm_mi_solve_cg(c, b.data(), q.data(), (int64_t) imax, (double) eps, r == 0 ? x.data() : sc[(size_t) r].data(),
                                    tr[(size_t) r].data(), &its[(size_t) r]);
            if (this->print_info_ && r == 0) (void) plssvm_mi_set_progress(c, nullptr, nullptr);
            return rc;
        });
        const int64_t it = its[0];
        iterations_ = it;
        trace_ = std::move(tr[0]);
        trace_.resize((std::size_t) it + 1);
        x.resize(b.size());
        if (this->print_info_) {
            const int64_t shown = std::min<int64_t>(it, (int64_t) imax);  // min(run + 1, imax)
            std::printf("Finished after %lld iterations with a residuum of %s (target: %s) and an average iteration time of %lldms.\n",
                        (long long) shown, shortest((T) trace_.back()).c_str(), shortest((T) ps.target).c_str(),
                        (long long) (shown > 0 ? ps.ms_total / (double) shown : 0.0));
            std::fflush(stdout);
        }
        return x;
    }
    // gpu_csvm::update_w (gpu_csvm.cpp:327-350): w_ = sum_i alpha_i x_i (linear model vector)
    void update_w() override {
        need_model();
        const size_t len = std::max<std::size_t>(this->num_features_, 1);
        this->w_.assign(len, T(0));
        auto sc = scratch(len);
        const T *alpha = this->alpha_ptr_->data();
        on_all([&](int r, plssvm_mi_ctx *c) {
            return plssvm_mi_update_w(c, alpha, r == 0 ? this->w_.data() : sc[(size_t) r].data());
        });
        this->w_.resize(this->num_features_);
    }
    // gpu_csvm::predict (gpu_csvm.cpp:52-127): decision values bias + sum_i alpha_i k(x_i, z) of dense points
    [[nodiscard]] std::vector<T> predict(const std::vector<std::vector<T>> &points) override {
        need_model();
        if (points.empty()) return {};
        std::vector<T> Z;
        Z.reserve(points.size() * points[0].size());
        for (const auto &z : points) {
            if (z.size() != points[0].size()) throw exception{ "All points in the data vector must have the same number of features!" };
            Z.insert(Z.end(), z.begin(), z.end());
        }
        std::vector<T> out(points.size());
        auto sc = scratch(points.size());
        const T *alpha = this->alpha_ptr_->data();
        on_all([&](int r, plssvm_mi_ctx *c) {
            return plssvm_mi_predict_dense(c, alpha, (double) this->bias_, Z.data(), (int64_t) points.size(),
                                           (int64_t) points[0].size(), r == 0 ? out.data() : sc[(size_t) r].data());
        });
        return out;
    }

    // ---- run_device_kernel + the mock_hip_csvm setters (tests/backends/HIP/mock_hip_csvm.hpp:24-51) ----
    void run_device_kernel(const std::vector<T> &q, std::vector<T> &ret, const std::vector<T> &d, T add) {
        std::vector<std::vector<T>> rets((size_t) grp_->size(), ret);  // every rank adds into its own copy
        on_all([&](int r, plssvm_mi_ctx *c) {
            return plssvm_mi_kp(c, q.data(), d.data(), r == 0 ? ret.data() : rets[(size_t) r].data(), (double) add);
        });
    }
    void set_cost(T c) {
        on_all([&](int, plssvm_mi_ctx *x) { return plssvm_mi_set_cost(x, (double) c); });
        this->cost_ = c;
    }
    // empty: the context's weights are cleared (those of an earlier learn() must not reach a later call)
    void apply_point_weights(const std::vector<T> &s) override {
        on_all([&](int, plssvm_mi_ctx *x) { return plssvm_mi_set_point_weights(x, s.empty() ? nullptr : s.data()); });
    }
    void set_QA_cost(T qa) {
        on_all([&](int, plssvm_mi_ctx *x) { return plssvm_mi_set_qa_cost(x, (double) qa); });
        this->QA_cost_ = qa;
    }

    // ---- one-vs-all models of K >= 2 classes (build-defined; the reference, v1.2.0, is binary only) ----
    // learn_multi: the classes are the distinct values of the parameter set's class_labels, ascending; per class
    // exactly learn() on +1 (the point is of the class) / -1, all classes in one plssvm_mi_learn_multi call on every rank
    void learn_multi() { learn_multi(this->num_features_); }
    void learn_multi(std::size_t imax) {
        const auto &p = this->params_;
        if (p.class_labels.empty()) throw exception{ "No labels given for training! Maybe the data is only usable for prediction?" };
        if (p.class_labels.size() != this->num_data_points_)
            throw exception{ "Number of labels (" + std::to_string(p.class_labels.size()) +
                             ") must match the number of data points (" + std::to_string(this->num_data_points_) + ")!" };
        std::vector<T> cls = p.class_labels;
        std::sort(cls.begin(), cls.end());
        cls.erase(std::unique(cls.begin(), cls.end()), cls.end());
        if (cls.size() < 2) throw exception{ "learn_multi needs at least 2 classes" };
        const size_t K = cls.size(), n = this->num_data_points_;
        std::vector<T> Y(K * n);
        for (size_t c = 0; c < K; ++c)
            for (size_t i = 0; i < n; ++i) Y[c * n + i] = p.class_labels[i] == cls[c] ? T(1) : T(-1);
        // class weights: class c's problem weighs its own points (the positives) by w[c], every other point by 1
        std::vector<T> S;
        if (!this->class_weights_.empty()) {
            S.assign(K * n, T(1));
            for (const auto &kv : this->class_weights_) {
                const auto it = std::lower_bound(cls.begin(), cls.end(), kv.first);
                if (it == cls.end() || *it != kv.first)
                    throw exception{ "class_weights: the label " + shortest(kv.first) + " does not occur in the data!" };
                const size_t c = (size_t) (it - cls.begin());
                for (size_t i = 0; i < n; ++i)
                    if (p.class_labels[i] == kv.first) S[c * n + i] = kv.second;
            }
        }
        if (!on_device_) setup_data_on_device();
        apply_point_weights({});  // the classes' weights travel in S; binary weights of an earlier learn() do not apply
        learn_lanes(Y, K, imax, nullptr, S.empty() ? nullptr : S.data(), (int64_t) n);
        classes_ = std::move(cls);
    }
    // learn() at every cost of `costs` (a search over C) in one plssvm_mi_learn_lanes call: row k of alphas() / biases()
    // / iterations_multi() / residual_traces() is learn() at costs[k], with the class weights if any are set
    void learn_costs(const std::vector<T> &costs) { learn_costs(costs, this->num_features_); }
    void learn_costs(const std::vector<T> &costs, std::size_t imax) {
        if (this->value_ptr_ == nullptr) throw exception{ "No labels given for training! Maybe the data is only usable for prediction?" };
        if (costs.empty()) throw exception{ "learn_costs needs at least one cost" };
        for (const T c : costs)
            if (!(c > T(0)) || !std::isfinite(c)) throw exception{ "learn_costs: every cost must be a finite number > 0!" };
        const std::vector<T> s = this->point_weights();
        const size_t K = costs.size(), n = this->num_data_points_;
        std::vector<T> Y(K * n);
        for (size_t k = 0; k < K; ++k) std::copy(this->value_ptr_->begin(), this->value_ptr_->end(), Y.begin() + k * n);
        if (!on_device_) setup_data_on_device();  // stored tiles and lanes of an earlier call are reused
        apply_point_weights(s);                   // the class weights, or none
        const std::vector<double> cd(costs.begin(), costs.end());
        learn_lanes(Y, K, imax, cd.data(), nullptr, 0);
        classes_.clear();
        costs_ = costs;
    }
    const std::vector<T> &costs() const { return costs_; }

    // k-fold cross-validation of the binary problem at every cost of `costs` (build-defined; LIBSVM's -v): the
    // nfold x costs.size() subset problems as lanes of one plssvm_mi_learn_held call over the setup's stored kernel
    // matrix, plssvm_mi_train_values, then every point's value from the model that did not see it. Returns the
    // accuracy per cost; held_values() / folds() keep the values [costs][n] and the fold of every point. One device;
    // the class weights apply as in learn_costs; no model is set.
    // stratified_folds: fold of point i = (its rank among the points of its label, in index order) mod nfold
    static std::vector<int64_t> stratified_folds(const std::vector<T> &labels, std::size_t nfold) {
        if (nfold < 2 || nfold > labels.size())
            throw exception{ "The number of folds (" + std::to_string(nfold) + ") must be between 2 and the number of data points (" +
                             std::to_string(labels.size()) + ")!" };
        std::map<T, int64_t> seen;
        std::vector<int64_t> folds(labels.size());
        for (size_t i = 0; i < labels.size(); ++i) folds[i] = seen[labels[i]]++ % (int64_t) nfold;
        return folds;
    }
    std::vector<double> cross_validate(std::size_t nfold, const std::vector<T> &costs) { return cross_validate(nfold, costs, this->num_features_); }
    std::vector<double> cross_validate(std::size_t nfold, const std::vector<T> &costs_in, std::size_t imax) {
        if (this->value_ptr_ == nullptr) throw exception{ "No labels given for training! Maybe the data is only usable for prediction?" };
        if (grp_->size() != 1) throw exception{ "Cross-validation runs on one device!" };
        const std::vector<T> costs = costs_in.empty() ? std::vector<T>{ this->cost_ } : costs_in;
        for (const T c : costs)
            if (!(c > T(0)) || !std::isfinite(c)) throw exception{ "cross_validate: every cost must be a finite number > 0!" };
        const std::vector<T> &y = *this->value_ptr_;
        const size_t n = this->num_data_points_, C = costs.size(), K = C * nfold;
        folds_ = stratified_folds(y, nfold);
        const std::vector<T> s = this->point_weights();
        std::vector<T> Y(K * n), al(K * n), out(K * n);
        std::vector<uint8_t> H(K * n);
        std::vector<double> cd(K), bi(K);
        std::vector<int64_t> its(K), piv(K);
        for (size_t k = 0; k < K; ++k) {  // lane = cost * nfold + fold
            std::copy(y.begin(), y.end(), Y.begin() + k * n);
            cd[k] = (double) costs[k / nfold];
            for (size_t i = 0; i < n; ++i) H[k * n + i] = folds_[i] == (int64_t) (k % nfold) ? 1 : 0;
        }
        if (!on_device_) setup_data_on_device();
        apply_point_weights(s);
        on_all([&](int, plssvm_mi_ctx *c) {
            const int rc = plssvm_mi_learn_held(c, Y.data(), (int64_t) K, (int64_t) n, cd.data(), nullptr, 0, H.data(), (int64_t) n,
                                                (int64_t) imax, (double) this->epsilon_, al.data(), bi.data(), nullptr, its.data(),
                                                piv.data());
            if (rc != PLSSVM_MI_OK) return rc;
            return plssvm_mi_train_values(c, al.data(), (int64_t) K, (int64_t) n, bi.data(), out.data(), (int64_t) n);
        });
        held_values_.assign(C * n, T(0));
        std::vector<double> acc(C);
        for (size_t c = 0; c < C; ++c) {
            size_t ok = 0;
            for (size_t i = 0; i < n; ++i) {
                const T v = out[(c * nfold + (size_t) folds_[i]) * n + i];
                held_values_[c * n + i] = v;
                ok += (v > T(0) ? T(1) : T(-1)) == (y[i] > T(0) ? T(1) : T(-1));
            }
            acc[c] = (double) ok / (double) n;
        }
        cv_iterations_ = std::move(its);
        return acc;
    }
    const std::vector<T> &held_values() const { return held_values_; }  // [costs][n], row-major
    const std::vector<int64_t> &folds() const { return folds_; }
    const std::vector<int64_t> &cv_iterations() const { return cv_iterations_; }  // [costs][nfold]

  private:
    // plssvm_mi_learn_lanes on every rank; the results of rank 0 into alphas_, biases_, iterations_multi_, traces_
    void learn_lanes(const std::vector<T> &Y, size_t K, std::size_t imax, const double *costs, const T *S, int64_t lds) {
        const size_t n = this->num_data_points_;
        const size_t R = (size_t) grp_->size();
        std::vector<std::vector<T>> al(R, std::vector<T>(K * n));
        std::vector<std::vector<double>> bi(R, std::vector<double>(K)), tr(R, std::vector<double>(K * (imax + 1), 0.0));
        std::vector<std::vector<int64_t>> its(R, std::vector<int64_t>(K, 0));
        on_all([&](int r, plssvm_mi_ctx *c) {
            return plssvm_mi_learn_lanes(c, Y.data(), (int64_t) K, (int64_t) n, costs, S, lds, (int64_t) imax,
                                         (double) this->epsilon_, al[(size_t) r].data(), bi[(size_t) r].data(),
                                         tr[(size_t) r].data(), its[(size_t) r].data());
        });
        alphas_ = std::move(al[0]);
        biases_.assign(bi[0].begin(), bi[0].end());
        iterations_multi_ = std::move(its[0]);
        traces_.clear();
        for (size_t c = 0; c < K; ++c)
            traces_.emplace_back(tr[0].begin() + c * (imax + 1), tr[0].begin() + c * (imax + 1) + iterations_multi_[c] + 1);
    }

  public:
    // the model of a one-vs-all model file: classes [K], alphas [K][n] (row-major), rhos [K]
    void set_model_multi(std::vector<T> classes, std::vector<T> alphas, const std::vector<T> &rhos) {
        if (classes.empty() || rhos.size() != classes.size() || alphas.size() != classes.size() * this->num_data_points_)
            throw exception{ "Number of weights (" + std::to_string(alphas.size()) + ") must match the number of classes (" +
                             std::to_string(classes.size()) + ") times the number of data points (" +
                             std::to_string(this->num_data_points_) + ")!" };
        classes_ = std::move(classes);
        alphas_ = std::move(alphas);
        biases_.clear();
        for (const T r : rhos) biases_.push_back(-r);
    }
    // decision values [K][np] (row-major) of the points held by `points` (dense or CSR): every class in one call
    std::vector<T> predict_values_multi(const parameter<T> &points) {
        if (classes_.empty()) throw exception{ "No alphas provided for prediction!" };
        if (!on_device_) setup_data_on_device();
        const int64_t K = (int64_t) classes_.size(), np = points.num_data_points, n = (int64_t) this->num_data_points_;
        const size_t len = (size_t) (K * std::max<int64_t>(np, 1));
        std::vector<T> out(len);
        auto sc = scratch(len);
        const std::vector<double> b(biases_.begin(), biases_.end());
        on_all([&](int r, plssvm_mi_ctx *c) {
            T *o = r == 0 ? out.data() : sc[(size_t) r].data();
            if (points.sparse)
                return plssvm_mi_predict_multi_csr(c, alphas_.data(), K, n, b.data(), points.rowptr.data(), points.col.data(),
                                                   points.val.data(), PLSSVM_MI_VAL_REAL, np, points.num_features, o,
                                                   std::max<int64_t>(np, 1));
            return plssvm_mi_predict_multi_dense(c, alphas_.data(), K, n, b.data(), points.dense.data(), np,
                                                 points.num_features, o, std::max<int64_t>(np, 1));
        });
        return out;
    }
    // the class with the largest decision value, the lowest class index on a tie
    std::vector<T> predict_label_multi(const parameter<T> &points) {
        const std::vector<T> v = predict_values_multi(points);
        const size_t K = classes_.size(), np = (size_t) points.num_data_points;
        std::vector<T> l(np);
        for (size_t p = 0; p < np; ++p) {
            size_t best = 0;
            for (size_t c = 1; c < K; ++c)
                if (v[c * np + p] > v[best * np + p]) best = c;
            l[p] = classes_[best];
        }
        return l;
    }
    // fraction of the points whose predicted label equals points.class_labels
    T accuracy_multi(const parameter<T> &points) {
        if (points.class_labels.empty()) throw exception{ "No labels given for the accuracy calculation!" };
        const std::vector<T> l = predict_label_multi(points);
        if (l.size() != points.class_labels.size())
            throw exception{ "Number of data points to predict and correct labels mismatch!" };
        std::size_t ok = 0;
        for (std::size_t i = 0; i < l.size(); ++i) ok += l[i] == points.class_labels[i];
        return (T) ok / (T) l.size();
    }
    const std::vector<T> &classes() const { return classes_; }
    const std::vector<T> &alphas() const { return alphas_; }  // [K][n], row-major
    const std::vector<T> &biases() const { return biases_; }
    const std::vector<int64_t> &iterations_multi() const { return iterations_multi_; }
    const std::vector<std::vector<double>> &residual_traces() const { return traces_; }

    // csvm<T>::write_model (src/plssvm/csvm.cpp:60-204): positive-label support vectors first. After learn_multi /
    // set_model_multi with three or more classes: the one-vs-all layout (parameter<T>::model_text_multi); two classes
    // are a binary model and are written by learn()
    void write_model(const std::string &filename) const {
        if (classes_.size() >= 3) {
            const auto &p = this->params_;
            if (p.class_labels.size() != this->num_data_points_)
                throw exception{ "No class labels given! A one-vs-all model file needs the class of every support vector." };
            std::vector<int64_t> pc(p.class_labels.size());
            for (size_t i = 0; i < pc.size(); ++i)
                pc[i] = (int64_t) (std::lower_bound(classes_.begin(), classes_.end(), p.class_labels[i]) - classes_.begin());
            std::vector<std::vector<T>> al;
            for (size_t c = 0; c < classes_.size(); ++c)
                al.emplace_back(alphas_.begin() + c * this->num_data_points_, alphas_.begin() + (c + 1) * this->num_data_points_);
            write_text(filename, p.model_text_multi(classes_, pc, al, biases_));
            return;
        }
        if (this->alpha_ptr_ == nullptr) throw exception{ "No alphas given! Maybe a call to 'learn()' is missing?" };
        const auto &p = this->params_;
        const auto &alpha_ = *this->alpha_ptr_;
        const T bias_ = this->bias_;
        std::size_t npos = 0, nneg = 0;
        for (const T v : p.labels) (v > 0 ? npos : nneg) += 1;
        std::string out = "svm_type c_svc\nkernel_type ";
        out += kernel_name(p.kernel);
        out += "\n";
        if (p.kernel == kernel_type::polynomial) {
            out += "degree " + std::to_string(p.degree) + "\ngamma " + shortest(p.gamma) + "\ncoef0 " + shortest(p.coef0) + "\n";
        } else if (p.kernel == kernel_type::rbf || p.kernel == kernel_type::laplacian) {
            out += "gamma " + shortest(p.gamma) + "\n";
        }
        out += "nr_class 2\ntotal_sv " + std::to_string(npos + nneg) + "\nrho " + shortest(-bias_) +
               "\nlabel 1 -1\nnr_sv " + std::to_string(npos) + " " + std::to_string(nneg) + "\nSV\n";
        for (int pass = 0; pass < 2; ++pass) {
            for (int64_t i = 0; i < p.num_data_points; ++i) {
                if ((p.labels[(std::size_t) i] > 0) != (pass == 0)) continue;
                out += shortest(alpha_[(std::size_t) i]) + " ";
                char buf[64];
                auto feat = [&](int64_t f, T v) {
                    std::snprintf(buf, sizeof buf, "%lld:%e ", (long long) f, (double) v);  // "{}:{:e} "
                    out += buf;
                };
                if (p.sparse) {
                    for (int64_t k = p.rowptr[i]; k < p.rowptr[i + 1]; ++k)
                        if (p.val[(std::size_t) k] != T(0)) feat(p.col[(std::size_t) k], p.val[(std::size_t) k]);
                } else {
                    for (int64_t f = 0; f < p.num_features; ++f)
                        if (p.dense[(std::size_t) (i * p.num_features + f)] != T(0)) feat(f, p.dense[(std::size_t) (i * p.num_features + f)]);
                }
                out += "\n";
            }
        }
        write_text(filename, out);
    }

    // model use (csvm.hpp:123-178; gpu_csvm::update_w / predict, gpu_csvm.cpp:52-127,327-350). Without a
    // preceding learn(), set_model() supplies the alphas and rho of a model file.
    void set_model(std::vector<T> alpha, T rho) {
        if (alpha.size() != this->num_data_points_)
            throw exception{ "Number of weights (" + std::to_string(alpha.size()) + ") must match the number of data points (" +
                             std::to_string(this->num_data_points_) + ")!" };
        this->alpha_ptr_ = std::make_shared<const std::vector<T>>(std::move(alpha));
        this->bias_ = -rho;
        this->w_.clear();
    }
    // decision values bias + sum_i alpha_i k(sv_i, z) of the points held by `points` (dense or CSR)
    std::vector<T> predict(const parameter<T> &points) {
        need_model();
        const size_t len = (std::size_t) std::max<int64_t>(points.num_data_points, 1);
        std::vector<T> out(len);
        auto sc = scratch(len);
        const T *alpha = this->alpha_ptr_->data();
        on_all([&](int r, plssvm_mi_ctx *c) {
            T *o = r == 0 ? out.data() : sc[(size_t) r].data();
            if (points.sparse)
                return plssvm_mi_predict_csr(c, alpha, (double) this->bias_, points.rowptr.data(), points.col.data(),
                                             points.val.data(), PLSSVM_MI_VAL_REAL, points.num_data_points,
                                             points.num_features, o);
            return plssvm_mi_predict_dense(c, alpha, (double) this->bias_, points.dense.data(), points.num_data_points,
                                           points.num_features, o);
        });
        out.resize((std::size_t) points.num_data_points);
        return out;
    }
    // csvm::predict_label: sign of the decision values (operators.hpp:174-177)
    std::vector<T> predict_label(const parameter<T> &points) {
        std::vector<T> v = predict(points);
        for (T &x : v) x = x > T(0) ? T(1) : T(-1);
        return v;
    }
    // csvm::accuracy(points, correct_labels)
    T accuracy(const parameter<T> &points) {
        if (points.labels.empty()) throw exception{ "No labels given for the accuracy calculation!" };
        const std::vector<T> l = predict_label(points);
        if (l.size() != points.labels.size())
            throw exception{ "Number of data points to predict and correct labels mismatch!" };
        std::size_t ok = 0;
        for (std::size_t i = 0; i < l.size(); ++i) ok += l[i] * points.labels[i] > T(0);
        return (T) ok / (T) l.size();
    }

    const std::vector<T> &alpha() const { return *this->alpha_ptr_; }
    const std::vector<T> &w() const { return this->w_; }
    T bias() const { return this->bias_; }
    T rho() const { return -this->bias_; }
    T QA_cost() const { return this->QA_cost_; }
    int64_t iterations() const { return iterations_; }
    const std::vector<double> &residual_trace() const { return trace_; }

    static std::string shortest(T v) { return plssvm::mi355x::shortest(v); }  // fmt "{}": shortest round-trip form

  private:
    static void write_text(const std::string &filename, const std::string &out) {
        std::FILE *fp = std::fopen(filename.c_str(), "w");
        if (!fp) throw std::runtime_error("Can't open model file '" + filename + "'!");
        std::fwrite(out.data(), 1, out.size(), fp);
        std::fclose(fp);
    }
    struct progress_state {
        int64_t imax;
        double target, ms_total;
        int64_t printed;
    };
    static void print_progress(int64_t first, int64_t count, const double *deltas, double target, double batch_ms, void *user) {
        auto &ps = *static_cast<progress_state *>(user);
        ps.target = target;
        const double per = batch_ms / (double) count;
        for (int64_t k = 0; k < count; ++k) {
            std::printf("Start Iteration %lld (max: %lld) with current residuum %s (target: %s). Done in %lldms.\n",
                        (long long) (first + k + 1), (long long) ps.imax, shortest((T) deltas[k]).c_str(),
                        shortest((T) target).c_str(), (long long) per);
        }
        ps.ms_total += (double) (long long) per * (double) count;
        ps.printed += count;
        std::fflush(stdout);
    }
    void need_model() {
        if (this->alpha_ptr_ == nullptr) throw exception{ "No alphas provided for prediction!" };
        if (!on_device_) setup_data_on_device();
    }
    // f(rank, ctx) -> PLSSVM_MI_* code on every rank at once; the first failing rank's message is thrown
    template <typename F>
    void on_all(F &&f) {
        try {
            grp_->run([&](int r, plssvm_mi_ctx *&c) { return f(r, c); });
        } catch (const group_error &e) {
            throw backend_exception(e.code, e.what());
        }
    }
    // host output buffers of the ranks other than 0 (their results equal rank 0's)
    std::vector<std::vector<T>> scratch(size_t len) const {
        std::vector<std::vector<T>> v((size_t) grp_->size());
        for (size_t r = 1; r < v.size(); ++r) v[r].assign(len, T(0));
        return v;
    }
    std::unique_ptr<device_group> grp_;
    std::vector<double> trace_;
    int64_t iterations_ = 0;
    bool on_device_ = false;
    // the one-vs-all model (learn_multi / set_model_multi)
    std::vector<T> classes_, alphas_, biases_, costs_;  // costs_: learn_costs' grid (then classes_ is empty)
    std::vector<T> held_values_;  // cross_validate
    std::vector<int64_t> folds_, cv_iterations_;
    std::vector<int64_t> iterations_multi_;
    std::vector<std::vector<double>> traces_;
};

}  // namespace plssvm::mi355x
