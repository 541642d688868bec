// bigconst.cpp -- clear multi-word arithmetic on public constants (bigconst.h).
#include "bigconst.h"

#include <algorithm>

namespace fhe {

BigConst big_norm(BigConst v) {
    while (!v.empty() && v.back() == 0) v.pop_back();
    return v;
}
uint32_t big_bitlen(const BigConst& v) {
    for (size_t w = v.size(); w-- > 0;)
        if (v[w]) return (uint32_t)(64 * w + 64 - __builtin_clzll(v[w]));
    return 0;
}
bool big_bit(const BigConst& v, uint32_t i) { return i / 64 < v.size() && ((v[i / 64] >> (i % 64)) & 1); }
int big_cmp(const BigConst& a, const BigConst& b) {
    const size_t n = std::max(a.size(), b.size());
    for (size_t w = n; w-- > 0;) {
        const uint64_t x = w < a.size() ? a[w] : 0, y = w < b.size() ? b[w] : 0;
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}
BigConst big_pow2(uint32_t e) {
    BigConst v(e / 64 + 1, 0);
    v[e / 64] = 1ull << (e % 64);
    return v;
}
BigConst big_add(const BigConst& a, const BigConst& b) {
    BigConst r(std::max(a.size(), b.size()) + 1, 0);
    unsigned __int128 c = 0;
    for (size_t w = 0; w < r.size(); ++w) {
        c += (unsigned __int128)(w < a.size() ? a[w] : 0) + (w < b.size() ? b[w] : 0);
        r[w] = (uint64_t)c;
        c >>= 64;
    }
    return big_norm(r);
}
void big_sub_inplace(BigConst& a, const BigConst& b) {  // a >= b
    uint64_t borrow = 0;
    for (size_t w = 0; w < a.size(); ++w) {
        const uint64_t y = w < b.size() ? b[w] : 0;
        const uint64_t d = a[w] - y - borrow;
        borrow = (a[w] < y || (a[w] == y && borrow)) ? 1 : 0;
        a[w] = d;
    }
}
BigConst big_shr1(BigConst v) {
    for (size_t w = 0; w < v.size(); ++w) v[w] = (v[w] >> 1) | (w + 1 < v.size() ? v[w + 1] << 63 : 0);
    return big_norm(v);
}
// floor(num / den), binary long division
BigConst big_div(const BigConst& num, const BigConst& den) {
    const uint32_t nb = big_bitlen(num);
    BigConst q((nb + 63) / 64 + 1, 0), r;
    for (uint32_t i = nb; i-- > 0;) {
        uint64_t carry = big_bit(num, i) ? 1 : 0;  // r = 2 r + bit i of num
        for (size_t w = 0; w < r.size(); ++w) {
            const uint64_t nc = r[w] >> 63;
            r[w] = (r[w] << 1) | carry;
            carry = nc;
        }
        if (carry) r.push_back(carry);
        if (big_cmp(r, den) >= 0) {
            big_sub_inplace(r, den);
            r = big_norm(r);
            q[i / 64] |= 1ull << (i % 64);
        }
    }
    return big_norm(q);
}
BigConst big_mul(const BigConst& x, const BigConst& y) {
    BigConst r(x.size() + y.size() + 1, 0);
    for (size_t i = 0; i < x.size(); ++i) {
        unsigned __int128 c = 0;
        for (size_t j = 0; j < y.size(); ++j) {
            c += (unsigned __int128)x[i] * y[j] + r[i + j];
            r[i + j] = (uint64_t)c;
            c >>= 64;
        }
        for (size_t k = i + y.size(); c; ++k) {
            c += r[k];
            r[k] = (uint64_t)c;
            c >>= 64;
        }
    }
    return big_norm(r);
}
BigConst big_shr(const BigConst& v, uint32_t s) {
    BigConst r;
    for (size_t w = s / 64; w < v.size(); ++w) {
        uint64_t x = v[w] >> (s % 64);
        if (s % 64 && w + 1 < v.size()) x |= v[w + 1] << (64 - s % 64);
        r.push_back(x);
    }
    return big_norm(r);
}
BigConst big_min(const BigConst& a, const BigConst& b) { return big_cmp(a, b) <= 0 ? a : b; }
BigConst big_mod(const BigConst& a, const BigConst& n) {
    if (big_cmp(a, n) < 0) return big_norm(a);
    BigConst r = a;
    big_sub_inplace(r, big_mul(big_div(a, n), n));
    return big_norm(r);
}
// sum_q v[q] 4^q for nonnegative v
BigConst big_from_digits(const std::vector<int64_t>& v) {
    BigConst D;
    auto shl2 = [](const BigConst& x) { return big_add(big_add(x, x), big_add(x, x)); };
    for (size_t q = v.size(); q-- > 0;) D = big_add(shl2(D), BigConst{(uint64_t)v[q]});
    return big_norm(D);
}

}  // namespace fhe
