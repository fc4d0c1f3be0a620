// TEST INFRASTRUCTURE: drives the field and curve primitives (the host path = the device source) through the op table of
// field_ops.h on operands read from stdin, so that tests/test_f29.py and tests/test_field_ops.py can compare them with
// Python integers at the extreme operands, and tests/test_field_probe_gpu.py can compare the device probe's words with these.
// Line format:  <target> <op> <na words of a> <nb words of b>   ->   no words of the result
// (for the lazy field ops na = nb = L limbs, as it has always been).  `f29_check --list` prints the table:
//   <target> <target id> <op> <op id> <na> <nb> <no>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "field_ops.h"
using namespace zkt;

static bool read_words(std::vector<uint32_t>& v, int n) {
    v.assign(n, 0);
    for (int i = 0; i < n; i++)
        if (scanf("%u", &v[i]) != 1) return false;
    return true;
}

static bool finish(const Shape& s, const std::vector<uint32_t>& o) {
    for (int i = 0; i < s.no; i++) printf("%u ", o[i]);
    printf("\n");
    return true;
}

template <class P>
static bool run_field(const char* opname) {
    for (int op = 0; op < F_COUNT; op++) {
        const Shape s = field_shape<P>(op);
        if (!s.ok || strcmp(opname, field_op_name(op))) continue;
        std::vector<uint32_t> a, b, o(s.no, 0);
        if (!read_words(a, s.na) || !read_words(b, s.nb)) return false;
        field_dispatch<P>(op, [&](auto id) { field_op<P, decltype(id)::value>(a.data(), b.data(), o.data()); });
        return finish(s, o);
    }
    printf("bad op\n");
    return false;
}

template <class CC>
static bool run_curve(const char* opname) {
    for (int op = 0; op < C_COUNT; op++) {
        const Shape s = curve_shape<CC>(op);
        if (!s.ok || strcmp(opname, curve_op_name(op))) continue;
        std::vector<uint32_t> a, b, o(s.no, 0);
        if (!read_words(a, s.na) || !read_words(b, s.nb)) return false;
        curve_dispatch<CC>(op, [&](auto id) { curve_op<CC, decltype(id)::value>(a.data(), b.data(), o.data()); });
        return finish(s, o);
    }
    printf("bad op\n");
    return false;
}

template <class P>
static void list_field(const char* name, int id) {
    for (int op = 0; op < F_COUNT; op++) {
        const Shape s = field_shape<P>(op);
        if (s.ok) printf("%s %d %s %d %d %d %d\n", name, id, field_op_name(op), op, s.na, s.nb, s.no);
    }
}
template <class CC>
static void list_curve(const char* name, int id) {
    for (int op = 0; op < C_COUNT; op++) {
        const Shape s = curve_shape<CC>(op);
        if (s.ok) printf("%s %d %s %d %d %d %d\n", name, id, curve_op_name(op), op, s.na, s.nb, s.no);
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--list")) {
#define X(i, P) list_field<P>(#P, i);
        ZK_PROBE_FIELDS(X)
#undef X
#define X(i, C)                                             \
    list_curve<C>(#C, CURVE_TARGET0 + 2 * i);               \
    list_curve<F29View<C>>(#C "29", CURVE_TARGET0 + 2 * i + 1);
        ZK_PROBE_CURVES(X)
#undef X
        return 0;
    }
    char target[32], op[32];
    while (scanf("%31s %31s", target, op) == 2) {
#define X(i, P)                           \
    if (!strcmp(target, #P)) {            \
        if (!run_field<P>(op)) return 1;  \
        continue;                         \
    }
        ZK_PROBE_FIELDS(X)
#undef X
#define X(i, C)                                       \
    if (!strcmp(target, #C)) {                        \
        if (!run_curve<C>(op)) return 1;              \
        continue;                                     \
    }                                                 \
    if (!strcmp(target, #C "29")) {                   \
        if (!run_curve<F29View<C>>(op)) return 1;     \
        continue;                                     \
    }
        ZK_PROBE_CURVES(X)
#undef X
        printf("bad target\n");
        return 1;
    }
    return 0;
}
