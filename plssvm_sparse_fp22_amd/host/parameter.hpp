// plssvm::mi355x::parameter<T> — training parameters + LIBSVM reader (C++17, host only).
//
// Mirrors plssvm::parameter<T> (include/plssvm/parameter.hpp:181-194 defaults; src/plssvm/parameter.cpp):
//   * LIBSVM lines left-trimmed, empty and '#' lines skipped (src/plssvm/detail/file_reader.cpp:129-153);
//   * label = token before the first space if it has no ':' (parameter.cpp:56-63), mapped by
//     sign (x > 0 ? +1 : -1, parameter.cpp:160-163);
//   * indices 0-based as written (parameter.cpp:75-83); num_features = max index + 1;
//   * gamma = 1 / num_features in the real type when not given (parameter.cpp:150-152);
//   * model file name = basename(input) + ".model", prediction file basename(input) + ".predict"
//     (parameter.cpp:575-584);
//   * model files as written by csvm::write_model (parameter.cpp:366-520).
// Unlike the reference, which always densifies, the data can be kept as CSR (`sparse = true`).
// Build-defined (the reference, v1.2.0, is binary only): `multiclass` keeps the raw label values (class_labels), and
// a model file with nr_class >= 3 holds a one-vs-all model (model_text_multi below states the layout).
#pragma once

#include <algorithm>
#include <cctype>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <string_view>
#include <type_traits>
#include <utility>
#include <vector>

namespace plssvm::mi355x {

// upstream's numbering; 3 (sigmoid) is not offered
enum class kernel_type { linear = 0, polynomial = 1, rbf = 2, laplacian = 4 };

inline const char *kernel_name(kernel_type k) {
    switch (k) {
        case kernel_type::linear: return "linear";
        case kernel_type::polynomial: return "polynomial";
        case kernel_type::laplacian: return "laplacian";
        default: return "rbf";
    }
}

inline kernel_type parse_kernel(std::string s) {
    std::transform(s.begin(), s.end(), s.begin(), [](unsigned char c) { return (char) std::tolower(c); });
    if (s == "linear" || s == "0") return kernel_type::linear;
    if (s == "polynomial" || s == "1") return kernel_type::polynomial;
    if (s == "rbf" || s == "2") return kernel_type::rbf;
    if (s == "laplacian" || s == "4") return kernel_type::laplacian;
    throw std::invalid_argument("Unrecognized kernel type '" + s + "'!");
}

// plssvm::invalid_file_format_exception / file_not_found_exception (include/plssvm/exceptions/exceptions.hpp)
struct invalid_file_format_exception : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct file_not_found_exception : std::runtime_error {
    using std::runtime_error::runtime_error;
};

template <typename T>
constexpr const char *arithmetic_type_name() {  // include/plssvm/detail/arithmetic_type_name.hpp
    if constexpr (std::is_same_v<T, float>) return "float";
    else if constexpr (std::is_same_v<T, double>) return "double";
    else if constexpr (std::is_same_v<T, int>) return "int";
    else if constexpr (std::is_same_v<T, unsigned int>) return "unsigned int";
    else if constexpr (std::is_same_v<T, unsigned long>) return "unsigned long";
    else return "unsigned long long";
}

// detail::convert_to (include/plssvm/detail/string_conversion.hpp:39-64): leading whitespace skipped, the
// longest valid prefix converted (std::from_chars; correctly rounded like fast_float), error message verbatim
template <typename T>
T convert_to(std::string_view sv) {
    while (!sv.empty() && std::isspace((unsigned char) sv.front())) sv.remove_prefix(1);
    T v{};
    const auto r = std::from_chars(sv.data(), sv.data() + sv.size(), v);
    if (r.ec != std::errc{})
        throw invalid_file_format_exception("Can't convert '" + std::string(sv) + "' to a value of type " +
                                            arithmetic_type_name<T>() + "!");
    return v;
}

// a whole token as a real (data values: trailing characters are an error)
template <typename T>
T to_real(std::string_view sv) {
    while (!sv.empty() && std::isspace((unsigned char) sv.front())) sv.remove_prefix(1);
    while (!sv.empty() && std::isspace((unsigned char) sv.back())) sv.remove_suffix(1);
    T v{};
    const auto r = std::from_chars(sv.data(), sv.data() + sv.size(), v);  // correctly rounded, like fast_float
    if (r.ec != std::errc{} || r.ptr != sv.data() + sv.size())
        throw invalid_file_format_exception("Can't convert '" + std::string(sv) + "' to a value of type " +
                                            arithmetic_type_name<T>() + "!");
    return v;
}

// fmt "{}" of a floating point value: the shortest round-trip form (std::to_chars)
template <typename T>
std::string shortest(T v) {
    char buf[64];
    const auto r = std::to_chars(buf, buf + sizeof buf, v);
    return std::string(buf, r.ptr);
}

template <typename T>
struct parameter {
    using real_type = T;
    kernel_type kernel = kernel_type::linear;
    int degree = 3;
    real_type gamma = 0;  // 0 -> 1 / num_features
    real_type coef0 = 0;
    real_type cost = 1;
    real_type epsilon = 0.001;
    bool print_info = true;
    std::string input_filename, model_filename;

    // data: dense rows (row-major n x d) or CSR
    bool sparse = false;
    int64_t num_data_points = 0, num_features = 0;
    std::vector<real_type> dense;
    std::vector<int64_t> rowptr;
    std::vector<int32_t> col;
    std::vector<real_type> val;
    std::vector<uint32_t> val22;    // packed FP22 words of `val` (binary FP22 input; kept packed for the device)
    std::vector<real_type> labels;  // +-1
    std::vector<real_type> class_labels;  // the label values as written (parse_*_file with multiclass = true)

    std::string predict_name_from_input() const {
        const auto pos = input_filename.find_last_of("/\\");
        return input_filename.substr(pos == std::string::npos ? 0 : pos + 1) + ".predict";
    }
    std::string model_name_from_input() const {
        const auto pos = input_filename.find_last_of("/\\");
        return input_filename.substr(pos == std::string::npos ? 0 : pos + 1) + ".model";
    }

    // LIBSVM rows "[label] idx:val ..." of content[start..] (parameter.cpp:40-176): left-trimmed, empty
    // and '#' lines skipped, a leading token without ':' is the label / alpha, indices 0-based
    struct rows_t {
        std::vector<std::vector<std::pair<int64_t, real_type>>> rows;
        std::vector<real_type> first;  // label (train / test) or alpha (model SV section)
        bool has_first = true;
    };
    static rows_t parse_rows(const std::string &content, std::size_t pos) {
        rows_t out;
        while (pos <= content.size()) {
            std::size_t nl = content.find('\n', pos);
            if (nl == std::string::npos) nl = content.size();
            std::string_view line(content.data() + pos, nl - pos);
            pos = nl + 1;
            while (!line.empty() && std::isspace((unsigned char) line.front())) line.remove_prefix(1);
            if (line.empty() || line.front() == '#') continue;
            std::size_t sp = line.find_first_of(" \n");
            const std::size_t colon = line.find_first_of(":\n");
            std::size_t p = 0;
            if (sp == std::string_view::npos) sp = line.size();
            if (colon == std::string_view::npos || colon >= sp) {
                out.first.push_back(to_real<real_type>(line.substr(0, sp)));
                p = sp;
            } else {
                out.has_first = false;
            }
            out.rows.push_back(parse_features(line, p));
        }
        return out;
    }
    // the "idx:val ..." entries of a line from position p on, sorted by index
    static std::vector<std::pair<int64_t, real_type>> parse_features(std::string_view line, std::size_t p) {
        std::vector<std::pair<int64_t, real_type>> r;
        while (true) {
            const std::size_t c = line.find(':', p);
            if (c == std::string_view::npos) break;
            std::string_view idx = line.substr(p, c - p);
            while (!idx.empty() && std::isspace((unsigned char) idx.front())) idx.remove_prefix(1);
            unsigned long index = 0;
            const auto res = std::from_chars(idx.data(), idx.data() + idx.size(), index);
            if (res.ec != std::errc{})
                throw invalid_file_format_exception("Can't convert '" + std::string(idx) +
                                                    "' to a value of type unsigned long!");
            p = c + 1;
            std::size_t e = line.find(' ', p);
            if (e == std::string_view::npos) e = line.size();
            r.emplace_back((int64_t) index, to_real<real_type>(line.substr(p, e - p)));
            p = e;
        }
        std::sort(r.begin(), r.end());
        return r;
    }

    static std::string read_file(const std::string &filename) {
        std::ifstream f(filename, std::ios::binary);
        if (!f) throw file_not_found_exception("Couldn't find file: '" + filename + "'!");
        std::stringstream ss;
        ss << f.rdbuf();
        return ss.str();
    }

    // the data of this parameter object from parsed rows (dense or CSR), d = max(min_features, max index + 1)
    void set_rows(const rows_t &pr, bool keep_sparse, int64_t min_features = 0) {
        const auto &rows = pr.rows;
        if (rows.empty()) throw invalid_file_format_exception("Can't parse file: no data points are given!");
        int64_t d = min_features;
        for (const auto &r : rows)
            if (!r.empty()) d = std::max<int64_t>(d, r.back().first + 1);
        if (d == 0) throw invalid_file_format_exception("Can't parse file: no data points are given!");
        num_data_points = (int64_t) rows.size();
        num_features = d;
        sparse = keep_sparse;
        rowptr.assign(1, 0);
        col.clear();
        val.clear();
        val22.clear();
        dense.clear();
        if (sparse) {
            for (const auto &r : rows) {
                for (const auto &[c, v] : r) {
                    col.push_back((int32_t) c);
                    val.push_back(v);
                }
                rowptr.push_back((int64_t) col.size());
            }
        } else {
            dense.assign((std::size_t) (num_data_points * d), real_type{ 0 });
            for (int64_t i = 0; i < num_data_points; ++i)
                for (const auto &[c, v] : rows[(std::size_t) i]) dense[(std::size_t) (i * d + c)] = v;
        }
    }

    // PLSSVMB1 binary CSR / FP22 data file (layout: plssvm_sparse_fp22_amd/io.py); always kept sparse
    static bool is_binary(const std::string &content) { return content.size() >= 48 && content.compare(0, 8, "PLSSVMB1") == 0; }
    void parse_binary(const std::string &c, bool multiclass = false) {
        auto rd = [&](std::size_t off, void *dst, std::size_t nb) {
            if (off + nb > c.size()) throw invalid_file_format_exception("truncated PLSSVMB1 file");
            std::memcpy(dst, c.data() + off, nb);
        };
        uint32_t vf[2];
        int64_t hdr[3];
        int32_t fmt[2];
        rd(8, vf, 8);
        rd(16, hdr, 24);
        rd(40, fmt, 8);
        if (vf[0] != 1) throw invalid_file_format_exception("unsupported PLSSVMB1 version");
        const int64_t n = hdr[0], d = hdr[1], nnz = hdr[2];
        if (n < 1 || d < 1 || nnz < 0) throw invalid_file_format_exception("Can't parse file: no data points are given!");
        auto pad8 = [](std::size_t b) { return (8 - b % 8) % 8; };
        std::size_t off = 48;
        rowptr.resize((std::size_t) n + 1);
        rd(off, rowptr.data(), 8 * ((std::size_t) n + 1));
        off += 8 * ((std::size_t) n + 1);
        col.resize((std::size_t) nnz);
        rd(off, col.data(), 4 * (std::size_t) nnz);
        off += 4 * (std::size_t) nnz + pad8(4 * (std::size_t) nnz);
        val.resize((std::size_t) nnz);
        val22.clear();
        std::size_t nb;
        if (fmt[0] == 2) {
            nb = 4 * 11 * (((std::size_t) nnz + 15) / 16);
            val22.resize(nb / 4 + 1, 0u);
            rd(off, val22.data(), nb);
            for (int64_t k = 0; k < nnz; ++k) {
                const int bit = 22 * (int) (k & 15);
                const uint32_t *w = val22.data() + (k >> 4) * 11 + (bit >> 5);
                const int sh = bit & 31;
                uint64_t x = (uint64_t) w[0] >> sh;
                if (sh > 10) x |= (uint64_t) w[1] << (32 - sh);
                const uint32_t u = (uint32_t) (x & 0x3FFFFFu) << 10;
                float f;
                std::memcpy(&f, &u, 4);
                val[(std::size_t) k] = (real_type) f;
            }
        } else if (fmt[0] == 1) {
            nb = 8 * (std::size_t) nnz;
            std::vector<double> tmp((std::size_t) nnz);
            rd(off, tmp.data(), nb);
            for (int64_t k = 0; k < nnz; ++k) val[(std::size_t) k] = (real_type) tmp[(std::size_t) k];
        } else {
            nb = 4 * (std::size_t) nnz;
            std::vector<float> tmp((std::size_t) nnz);
            rd(off, tmp.data(), nb);
            for (int64_t k = 0; k < nnz; ++k) val[(std::size_t) k] = (real_type) tmp[(std::size_t) k];
        }
        off += nb + pad8(nb);
        labels.clear();
        class_labels.clear();
        if (vf[1] & 1u) {
            std::vector<double> y((std::size_t) n);
            rd(off, y.data(), 8 * (std::size_t) n);
            for (const double v : y) labels.push_back(v > 0 ? real_type{ 1 } : real_type{ -1 });
            if (multiclass) class_labels.assign(y.begin(), y.end());
        }
        if (rowptr[0] != 0 || rowptr.back() != nnz) throw invalid_file_format_exception("corrupt PLSSVMB1 row pointers");
        sparse = true;
        num_data_points = n;
        num_features = d;
        dense.clear();
    }

    // parse_train_file -> parse_libsvm_file (src/plssvm/parameter.cpp:132-176); PLSSVMB1 binary files too
    // multiclass: the label values are kept as written in class_labels (labels still holds their signs)
    void parse_train_file(const std::string &filename, bool keep_sparse = false, bool multiclass = false) {
        if (model_filename.empty() || model_filename == model_name_from_input()) {
            input_filename = filename;
            model_filename = model_name_from_input();
        }
        input_filename = filename;
        const std::string content = read_file(filename);
        if (is_binary(content)) {
            parse_binary(content, multiclass);
            if (gamma == real_type{ 0 }) gamma = real_type{ 1 } / static_cast<real_type>(num_features);
            return;
        }
        const rows_t pr = parse_rows(content, 0);
        set_rows(pr, keep_sparse);
        if (gamma == real_type{ 0 }) gamma = real_type{ 1 } / static_cast<real_type>(num_features);
        set_labels(pr, multiclass);
    }

    // parse_test_file (parameter.cpp:132-176 on the test set): points + optional labels
    void parse_test_file(const std::string &filename, bool keep_sparse = false, int64_t min_features = 0,
                         bool multiclass = false) {
        const rows_t pr = parse_rows(read_file(filename), 0);
        set_rows(pr, keep_sparse, min_features);
        set_labels(pr, multiclass);
    }
    void set_labels(const rows_t &pr, bool multiclass) {
        labels.clear();
        class_labels.clear();
        if (pr.has_first && (int64_t) pr.first.size() == num_data_points) {
            for (const real_type v : pr.first) labels.push_back(v > real_type{ 0 } ? real_type{ 1 } : real_type{ -1 });
            if (multiclass) class_labels = pr.first;
        }
    }

    // parse_model_file (src/plssvm/parameter.cpp:366-520): the header lines (left-trimmed, '#' comments
    // skipped, lower-cased) until "sv", with the reference's checks and messages; then total_sv lines
    // "alpha idx:val ..." — the support vectors become this object's data, their alphas `alpha`, -rho the bias.
    // nr_class >= 3 (build-defined, parse_model_multi): classes, rhos and alphas [nr_class][total_sv] instead
    real_type rho = 0;
    std::vector<real_type> alpha;
    std::vector<int64_t> nr_sv;
    real_type label_first = 0, label_second = 0;
    int64_t nr_class = 2;
    std::vector<real_type> classes, rhos;
    std::vector<std::vector<real_type>> alphas;
    void parse_model_file(const std::string &filename, bool keep_sparse = false, int64_t min_features = 0) {
        const std::string content = read_file(filename);
        // lines as detail::file_reader keeps them (file_reader.cpp:129-153)
        std::vector<std::string_view> lines;
        for (std::size_t pos = 0; pos <= content.size();) {
            std::size_t nl = content.find('\n', pos);
            if (nl == std::string::npos) nl = content.size();
            std::string_view l(content.data() + pos, nl - pos);
            pos = nl + 1;
            while (!l.empty() && std::isspace((unsigned char) l.front())) l.remove_prefix(1);
            if (!l.empty() && l.front() != '#') lines.push_back(l);
        }
        // nr_class decides the layout: 2 is the reference's binary model (below), 3 or more the one-vs-all layout
        for (const std::string_view l : lines) {
            const std::string line = header_line(l);
            if (line == "sv") break;
            if (line.rfind("nr_class", 0) == 0 && convert_to<unsigned int>(header_value(line)) >= 3) {
                parse_model_multi(lines, keep_sparse, min_features);
                return;
            }
        }
        unsigned long long num_sv = 0;
        bool rho_set = false, nr_sv_set = false;
        label_first = label_second = 0;
        nr_class = 2;
        classes.clear();
        rhos.clear();
        alphas.clear();
        auto trim_left = [](std::string_view v) {
            while (!v.empty() && std::isspace((unsigned char) v.front())) v.remove_prefix(1);
            return v;
        };
        std::size_t header = 0;
        for (; header < lines.size(); ++header) {
            std::string_view raw = lines[header];
            while (!raw.empty() && std::isspace((unsigned char) raw.back())) raw.remove_suffix(1);
            const std::string line = header_line(raw);
            std::string_view value = header_value(line);
            auto starts = [&](const char *k) { return line.rfind(k, 0) == 0; };
            if (common_header_entry(line, value, num_sv)) {
            } else if (starts("nr_class")) {
                const auto k = convert_to<unsigned int>(value);
                if (k < 2)
                    throw invalid_file_format_exception("The number of classes must be at least 2, but is " +
                                                        std::to_string(k) + "!");
            } else if (starts("rho")) {
                rho = convert_to<real_type>(value);
                rho_set = true;
            } else if (starts("label")) {
                const std::string_view first = value.substr(0, value.find_first_of(' '));
                label_first = convert_to<real_type>(first);
                value.remove_prefix(std::min(first.size() + 1, value.size()));
                const std::string_view second = value.substr(0, value.find_first_of(" \n"));
                label_second = convert_to<real_type>(second);
                value.remove_prefix(std::min(second.size() + 1, value.size()));
                value = trim_left(value);
                if (!value.empty() || (label_first != 1 && label_first != -1) || (label_second != 1 && label_second != -1))
                    throw invalid_file_format_exception("Only the labels 1 and -1 are allowed, but '" + line +
                                                        "' were given!");
            } else if (starts("nr_sv")) {
                const std::string_view first = value.substr(0, value.find_first_of(' '));
                const auto a = convert_to<unsigned long long>(first);
                value.remove_prefix(std::min(first.size() + 1, value.size()));
                const std::string_view second = value.substr(0, value.find_first_of(" \n"));
                const auto b = convert_to<unsigned long long>(second);
                value.remove_prefix(std::min(second.size() + 1, value.size()));
                value = trim_left(value);
                if (!value.empty())
                    throw invalid_file_format_exception("Only two numbers are allowed, but more were given '" + line + "'!");
                if (a + b != num_sv)
                    throw invalid_file_format_exception(
                        "The number of positive and negative support vectors doesn't add up to the total number: " +
                        std::to_string(a) + " + " + std::to_string(b) + " != " + std::to_string(num_sv) + "!");
                nr_sv = { (int64_t) a, (int64_t) b };
                nr_sv_set = true;
            } else if (line == "sv") {
                break;
            } else {
                throw invalid_file_format_exception("Unrecognized header entry '" + std::string(raw) +
                                                    "'! Maybe SV is missing?");
            }
        }
        if (num_sv == 0) throw invalid_file_format_exception("Missing total number of support vectors!");
        if (label_first == 0 || label_second == 0) throw invalid_file_format_exception("Missing labels!");
        if (!nr_sv_set) throw invalid_file_format_exception("Missing number of support vectors per class!");
        if (!rho_set) throw invalid_file_format_exception("Missing rho value!");
        if (header + 1 >= lines.size())
            throw invalid_file_format_exception("Can't parse file: no support vectors are given or SV is missing!");
        if (lines.size() - header - 1 < num_sv)
            throw invalid_file_format_exception("total_sv is " + std::to_string(num_sv) + ", but only " +
                                                std::to_string(lines.size() - header - 1) +
                                                " support vectors are given!");
        // the support vector lines: exactly total_sv of them (parse_libsvm_content(f, header + 1, data(num_sv), ...))
        const std::size_t sv_begin = (std::size_t) (lines[header + 1].data() - content.data());
        const std::size_t sv_end = header + 1 + num_sv < lines.size()
                                       ? (std::size_t) (lines[header + 1 + num_sv].data() - content.data())
                                       : content.size();
        const rows_t pr = parse_rows(content.substr(0, sv_end), sv_begin);
        if (!pr.has_first || pr.first.size() != pr.rows.size())
            throw invalid_file_format_exception("Every support vector needs an alpha value!");
        set_rows(pr, keep_sparse, min_features);
        alpha = pr.first;
        if (gamma == real_type{ 0 }) gamma = real_type{ 1 } / static_cast<real_type>(num_features);
    }

    // a header line as compared: right-trimmed and lower-cased; its value: what follows the first space
    static std::string header_line(std::string_view raw) {
        while (!raw.empty() && std::isspace((unsigned char) raw.back())) raw.remove_suffix(1);
        std::string line(raw);
        std::transform(line.begin(), line.end(), line.begin(), [](unsigned char c) { return (char) std::tolower(c); });
        return line;
    }
    static std::string_view header_value(const std::string &line) {
        std::string_view value{ line };
        value.remove_prefix(std::min(value.find_first_of(' ') + 1, value.size()));
        while (!value.empty() && std::isspace((unsigned char) value.front())) value.remove_prefix(1);
        return value;
    }
    // the header entries both layouts share: svm_type, kernel_type, gamma, degree, coef0, total_sv
    bool common_header_entry(const std::string &line, std::string_view value, unsigned long long &num_sv) {
        auto starts = [&](const char *k) { return line.rfind(k, 0) == 0; };
        if (starts("svm_type")) {
            if (value != "c_svc")
                throw invalid_file_format_exception("Can only use c_svc as svm_type, but '" + std::string(value) +
                                                    "' was given!");
        } else if (starts("kernel_type")) {
            std::string_view tok = value.substr(0, value.find_first_of(' '));
            if (tok == "linear" || tok == "0") kernel = kernel_type::linear;
            else if (tok == "polynomial" || tok == "1") kernel = kernel_type::polynomial;
            else if (tok == "rbf" || tok == "2") kernel = kernel_type::rbf;
            else if (tok == "laplacian" || tok == "4") kernel = kernel_type::laplacian;
            else throw invalid_file_format_exception("Unrecognized kernel type '" + std::string(value) + "'!");
        } else if (starts("gamma")) {
            gamma = convert_to<real_type>(value);
        } else if (starts("degree")) {
            degree = convert_to<int>(value);
        } else if (starts("coef0")) {
            coef0 = convert_to<real_type>(value);
        } else if (starts("total_sv")) {
            num_sv = convert_to<unsigned long long>(value);
            if (num_sv == 0)
                throw invalid_file_format_exception("The number of support vectors must be greater than 0, but is 0!");
        } else {
            return false;
        }
        return true;
    }
    static std::vector<std::string_view> tokens(std::string_view v) {
        std::vector<std::string_view> t;
        while (true) {
            while (!v.empty() && std::isspace((unsigned char) v.front())) v.remove_prefix(1);
            if (v.empty()) return t;
            const std::size_t e = std::min(v.find_first_of(" \t"), v.size());
            t.push_back(v.substr(0, e));
            v.remove_prefix(e);
        }
    }

    // The one-vs-all model of nr_class = K >= 3 classes (model_text_multi writes it): "label" holds the K distinct class
    // labels, "rho" K values, "nr_sv" the points per class, and every support-vector line K coefficients before its
    // features. The support vectors become this object's data, `classes`, `rhos` and `alphas` [K][total_sv] the model.
    void parse_model_multi(const std::vector<std::string_view> &lines, bool keep_sparse, int64_t min_features) {
        unsigned long long num_sv = 0;
        unsigned int K = 0;
        std::string label_line, rho_line, nr_sv_line;
        bool label_set = false, rho_set = false, nr_sv_set = false;
        std::size_t header = 0;
        for (; header < lines.size(); ++header) {
            std::string_view raw = lines[header];
            while (!raw.empty() && std::isspace((unsigned char) raw.back())) raw.remove_suffix(1);
            const std::string line = header_line(raw);
            const std::string_view value = header_value(line);
            auto starts = [&](const char *k) { return line.rfind(k, 0) == 0; };
            if (common_header_entry(line, value, num_sv)) {
            } else if (starts("nr_class")) {
                K = convert_to<unsigned int>(value);
            } else if (starts("rho")) {
                rho_line = line, rho_set = true;
            } else if (starts("label")) {
                label_line = line, label_set = true;
            } else if (starts("nr_sv")) {
                nr_sv_line = line, nr_sv_set = true;
            } else if (line == "sv") {
                break;
            } else {
                throw invalid_file_format_exception("Unrecognized header entry '" + std::string(raw) +
                                                    "'! Maybe SV is missing?");
            }
        }
        if (num_sv == 0) throw invalid_file_format_exception("Missing total number of support vectors!");
        if (!label_set) throw invalid_file_format_exception("Missing labels!");
        if (!nr_sv_set) throw invalid_file_format_exception("Missing number of support vectors per class!");
        if (!rho_set) throw invalid_file_format_exception("Missing rho value!");
        // the counts against nr_class: labels first (a binary header that claims more classes keeps the reference's text)
        const auto lt = tokens(header_value(label_line)), rt = tokens(header_value(rho_line)), nt = tokens(header_value(nr_sv_line));
        if (lt.size() != K)
            throw invalid_file_format_exception("Can only use " + std::to_string(lt.size()) + " classes, but " +
                                                std::to_string(K) + " were given!");
        if (rt.size() != K)
            throw invalid_file_format_exception("The number of rho values must match the number of classes, but " +
                                                std::to_string(rt.size()) + " != " + std::to_string(K) + "!");
        if (nt.size() != K)
            throw invalid_file_format_exception("The number of support vector counts must match the number of classes, but " +
                                                std::to_string(nt.size()) + " != " + std::to_string(K) + "!");
        nr_class = (int64_t) K;
        classes.clear();
        rhos.clear();
        nr_sv.clear();
        unsigned long long sum = 0;
        std::string sum_text;
        for (unsigned int c = 0; c < K; ++c) {
            classes.push_back(convert_to<real_type>(lt[c]));
            rhos.push_back(convert_to<real_type>(rt[c]));
            const auto cnt = convert_to<unsigned long long>(nt[c]);
            nr_sv.push_back((int64_t) cnt);
            sum += cnt;
            sum_text += (c ? " + " : "") + std::to_string(cnt);
        }
        for (unsigned int c = 0; c < K; ++c) {
            if (!std::isfinite(classes[c]))
                throw invalid_file_format_exception("The labels must be finite, but '" + label_line + "' were given!");
            for (unsigned int e = 0; e < c; ++e)
                if (classes[e] == classes[c])
                    throw invalid_file_format_exception("The labels must be distinct, but '" + label_line + "' were given!");
        }
        if (sum != num_sv)
            throw invalid_file_format_exception("The number of support vectors per class doesn't add up to the total number: " +
                                                sum_text + " != " + std::to_string(num_sv) + "!");
        if (header + 1 >= lines.size())
            throw invalid_file_format_exception("Can't parse file: no support vectors are given or SV is missing!");
        if (lines.size() - header - 1 < num_sv)
            throw invalid_file_format_exception("total_sv is " + std::to_string(num_sv) + ", but only " +
                                                std::to_string(lines.size() - header - 1) + " support vectors are given!");
        rows_t pr;
        pr.has_first = false;
        alphas.assign(K, std::vector<real_type>());
        for (unsigned long long i = 0; i < num_sv; ++i) {
            const std::string_view line = lines[header + 1 + i];
            std::size_t p = 0;
            unsigned int got = 0;
            for (; got < K; ++got) {
                while (p < line.size() && line[p] == ' ') ++p;
                const std::size_t e = std::min(line.find(' ', p), line.size());
                const std::string_view tok = line.substr(p, e - p);
                if (tok.empty() || tok.find(':') != std::string_view::npos) break;
                alphas[got].push_back(to_real<real_type>(tok));
                p = e;
            }
            if (got < K)
                throw invalid_file_format_exception("Every support vector needs " + std::to_string(K) +
                                                    " alpha values, but support vector " + std::to_string(i + 1) + " has " +
                                                    std::to_string(got) + "!");
            pr.rows.push_back(parse_features(line, p));
        }
        set_rows(pr, keep_sparse, min_features);
        alpha.clear();
        rho = 0;
        labels.clear();
        if (gamma == real_type{ 0 }) gamma = real_type{ 1 } / static_cast<real_type>(num_features);
    }

    // The text of a one-vs-all model file (build-defined; the layout follows the one-vs-all models of later PLSSVM
    // releases): the header of csvm::write_model with "nr_class K", "label" the K classes ascending, "total_sv",
    // "nr_sv" the points per class and "rho" -bias_c in label order; then the support vectors grouped by class in
    // label order (file order inside a class), each line "alpha_0[i] ... alpha_{K-1}[i] idx:val ...". point_class[i]
    // is the class index of point i; alphas is [K][n].
    std::string model_text_multi(const std::vector<real_type> &cls, const std::vector<int64_t> &point_class,
                                 const std::vector<std::vector<real_type>> &al, const std::vector<real_type> &biases) const {
        const std::size_t K = cls.size();
        std::vector<std::size_t> count(K, 0);
        for (const int64_t c : point_class) count[(std::size_t) c] += 1;
        std::string out = "svm_type c_svc\nkernel_type ";
        out += kernel_name(kernel);
        out += "\n";
        if (kernel == kernel_type::polynomial) {
            out += "degree " + std::to_string(degree) + "\ngamma " + shortest(gamma) + "\ncoef0 " + shortest(coef0) + "\n";
        } else if (kernel == kernel_type::rbf || kernel == kernel_type::laplacian) {
            out += "gamma " + shortest(gamma) + "\n";
        }
        out += "nr_class " + std::to_string(K) + "\nlabel";
        for (const real_type c : cls) out += " " + shortest(c);
        out += "\ntotal_sv " + std::to_string(num_data_points) + "\nnr_sv";
        for (const std::size_t c : count) out += " " + std::to_string(c);
        out += "\nrho";
        for (const real_type b : biases) out += " " + shortest(-b);
        out += "\nSV\n";
        char buf[64];
        for (std::size_t c = 0; c < K; ++c) {
            for (int64_t i = 0; i < num_data_points; ++i) {
                if (point_class[(std::size_t) i] != (int64_t) c) continue;
                for (std::size_t k = 0; k < K; ++k) out += shortest(al[k][(std::size_t) i]) + " ";
                auto feat = [&](int64_t f, real_type v) {
                    std::snprintf(buf, sizeof buf, "%lld:%e ", (long long) f, (double) v);  // "{}:{:e} "
                    out += buf;
                };
                if (sparse) {
                    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
                        if (val[(std::size_t) k] != real_type{ 0 }) feat(col[(std::size_t) k], val[(std::size_t) k]);
                } else {
                    for (int64_t f = 0; f < num_features; ++f)
                        if (dense[(std::size_t) (i * num_features + f)] != real_type{ 0 }) feat(f, dense[(std::size_t) (i * num_features + f)]);
                }
                out += "\n";
            }
        }
        return out;
    }

    real_type value(int64_t i, int64_t f) const {  // feature f of point i (dense or CSR)
        if (!sparse) return dense[(std::size_t) (i * num_features + f)];
        const auto b = col.begin() + rowptr[i], e = col.begin() + rowptr[i + 1];
        const auto it = std::lower_bound(b, e, (int32_t) f);
        return (it != e && *it == f) ? val[(std::size_t) (it - col.begin())] : real_type{ 0 };
    }
};

}  // namespace plssvm::mi355x
