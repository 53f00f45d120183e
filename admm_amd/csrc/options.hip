// The named options of the library (options.h): names, parsing, the per-thread settings and the environment overlay.
#include <cctype>
#include <cerrno>
#include <cstring>
#include "admm_internal.h"

extern char** environ;

namespace admm {
namespace {

struct OptRow { const char* name; OptAccepts accepts; };
constexpr OptRow kRows[kNumOptions] = {
#define ADMM_OPT_ROW(id, accepts, summary) {#id, accepts},
    ADMM_OPTIONS(ADMM_OPT_ROW)
#undef ADMM_OPT_ROW
};

std::string accepted(const OptAccepts& a) {
    auto num = [](double v) { char b[32]; std::snprintf(b, sizeof(b), "%.17g", v); return std::string(b); };
    switch (a.kind) {
    case OptKind::Flag: return "0 or 1";
    case OptKind::Int: return "an integer in [" + num(a.lo) + ", " + num(a.hi) + "]";
    case OptKind::Real: return a.lo == kPositive ? "a number > 0" : "a number in [" + num(a.lo) + ", " + num(a.hi) + "]";
    case OptKind::Choice: return std::string("one of ") + a.choices;
    case OptKind::Text: return "a non-empty string";
    case OptKind::Sched: return "big,small,split with widths 32 .. 256 in steps of 32 and split 0 .. 1000";
    case OptKind::Devices: return "0, all, or a comma-separated list of device numbers";
    }
    return "";
}

// place of `v` in the list "a|b|c", or -1
int choice_index(const char* list, const char* v) {
    const size_t n = std::strlen(v);
    int k = 0;
    for (const char* s = list;; ++k) {
        const char* e = std::strchr(s, '|');
        const size_t len = e ? (size_t)(e - s) : std::strlen(s);
        if (len == n && std::strncmp(s, v, n) == 0) return k;
        if (!e) return -1;
        s = e + 1;
    }
}

bool parse_int(const char* t, long long* out) {
    if (!*t || std::isspace((unsigned char)*t)) return false;
    char* end = nullptr;
    errno = 0;
    *out = std::strtoll(t, &end, 10);
    return errno == 0 && *end == 0;
}

bool parse_real(const char* t, double* out) {
    if (!*t || std::isspace((unsigned char)*t)) return false;
    char* end = nullptr;
    *out = std::strtod(t, &end);
    return *end == 0 && std::isfinite(*out);
}

bool parse_sched(const char* t, int out[3]) {
    std::string s(t);
    long long v[3];
    size_t i = 0;
    for (int k = 0; k < 3; ++k) {
        const size_t j = k < 2 ? s.find(',', i) : s.size();
        if (j == std::string::npos || !parse_int(s.substr(i, j - i).c_str(), &v[k])) return false;
        i = j + 1;
    }
    for (int k = 0; k < 2; ++k) if (v[k] < 32 || v[k] > 256 || v[k] % 32 != 0) return false;      // 256: kSyCBMax (symv_kernels.h)
    if (v[2] < 0 || v[2] > 1000) return false;
    for (int k = 0; k < 3; ++k) out[k] = (int)v[k];
    return true;
}

// ADMM_HIP_<NAME> variables of the environment the library was first used in -- read once, never again.  Names not in the table
// belong to the build or the Python loader (ADMM_HIP_EXTRA_CXXFLAGS, ADMM_HIP_LIB) and are ignored; the first malformed value of
// a known name is kept as an error that every entry point reports.
struct Overlay {
    ThreadOptions opts;
    std::string error;
};
const Overlay& overlay() {
    static const Overlay* m = []() {
        Overlay* o = new Overlay();
        for (char** e = environ; e && *e; ++e) {
            if (std::strncmp(*e, "ADMM_HIP_", 9) != 0) continue;
            const char* eq = std::strchr(*e, '=');
            Opt id;
            if (!eq || !opt_find(std::string(*e, (size_t)(eq - *e)).c_str(), &id)) continue;
            try {
                opt_parse(id, eq + 1, &o->opts.v[(int)id]);
                o->opts.has[(int)id] = true;
            } catch (const Error& err) {
                if (o->error.empty()) o->error = std::string("environment variable ADMM_HIP_") + err.what();
            }
        }
        return o;
    }();
    return *m;
}

}  // namespace

bool opt_find(const char* name, Opt* id) {
    std::string n(name);
    if (n.rfind("ADMM_HIP_", 0) == 0) n = n.substr(9);
    for (char& c : n) c = (char)std::toupper((unsigned char)c);
    for (int k = 0; k < kNumOptions; ++k)
        if (n == kRows[k].name) { *id = (Opt)k; return true; }
    return false;
}

void opt_parse(Opt id, const char* text, OptValue* out) {
    const OptAccepts& a = kRows[(int)id].accepts;
    OptValue v;
    v.text = text;
    bool ok = false;
    switch (a.kind) {
    case OptKind::Flag:
    case OptKind::Int: ok = parse_int(text, &v.i) && v.i >= a.lo && v.i <= a.hi; break;
    case OptKind::Real: ok = parse_real(text, &v.r) && v.r >= a.lo && v.r <= a.hi; break;
    case OptKind::Choice: v.i = choice_index(a.choices, text); ok = v.i >= 0; break;
    case OptKind::Text: ok = text[0] != 0; break;
    case OptKind::Sched: ok = parse_sched(text, v.sched); break;
    case OptKind::Devices:
        try { (void)parse_par_devices(text, 10000); ok = true; } catch (const Error&) { ok = false; }      // device numbers: at most 4 digits
        break;
    }
    ADMM_REQUIRE(ok, std::string(kRows[(int)id].name) + "='" + text + "' is not accepted: the option takes " + accepted(a));
    *out = std::move(v);
}

ThreadOptions& thread_options() { static thread_local ThreadOptions t; return t; }

void opt_set_thread(Opt id, const char* value) {
    ThreadOptions& t = thread_options();
    if (!value) { t.has[(int)id] = false; t.v[(int)id] = OptValue(); return; }
    opt_parse(id, value, &t.v[(int)id]);
    t.has[(int)id] = true;
}

void check_option_overlay() {
    const Overlay& o = overlay();
    ADMM_REQUIRE(o.error.empty(), o.error);
}

const OptValue* opt(Opt id) {
    const ThreadOptions& t = thread_options();
    if (t.has[(int)id]) return &t.v[(int)id];
    const ThreadOptions& o = overlay().opts;
    return o.has[(int)id] ? &o.v[(int)id] : nullptr;
}

bool opt_is(Opt id, const char* choice) {
    const OptAccepts& a = kRows[(int)id].accepts;
    const int k = a.kind == OptKind::Choice ? choice_index(a.choices, choice) : -1;
    if (k < 0) throw Error(ADMM_ERR_INTERNAL, std::string("option ") + kRows[(int)id].name + " has no value '" + choice + "'");
    const OptValue* v = opt(id);
    return v && v->i == k;
}

std::vector<int> parse_par_devices(const char* v, int device_count) {
    std::vector<int> out;
    if (!v) return out;
    const std::string s(v);
    if (s.empty() || s == "0") return out;
    if (s == "all") {
        ADMM_REQUIRE(device_count >= 1, "PAR_DEVICES=all: no device");
        for (int d = 0; d < device_count && d < 64; ++d) out.push_back(d);
        return out;
    }
    size_t i = 0;
    while (i <= s.size()) {
        const size_t j = std::min(s.find(',', i), s.size());
        const std::string item = s.substr(i, j - i);
        ADMM_REQUIRE(!item.empty() && item.size() <= 4 && item.find_first_not_of("0123456789") == std::string::npos,
                     "PAR_DEVICES must be 0, all, or a comma-separated list of device numbers (got '" + s + "')");
        const int d = std::atoi(item.c_str());
        ADMM_REQUIRE(d < device_count, "PAR_DEVICES lists device " + item + " but there are " + std::to_string(device_count) + " devices");
        out.push_back(d);
        ADMM_REQUIRE(out.size() <= 64, "PAR_DEVICES lists more than 64 ranks");
        i = j + 1;
    }
    return out;
}

}  // namespace admm
