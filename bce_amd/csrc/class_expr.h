// class_expr.h -- the expression language of the class search (`bce -ge EXPR`, bce_amd.compile_classes speaks the same grammar in
// Python; tests/class_emul.cpp --parse compares the two): an expression over BYTES becomes one 256-bit class per position, the
// masks bce_hip_count_classes / _locate_classes take (8 words per class, byte c is bit c & 31 of word c >> 5).  Host only.
//
//   .            any byte
//   [...]        a set: bytes and ranges a-b (a > b is an error); a leading ^ negates.  Inside a set only ] \ and - are special
//                (and ^ in front); a - that is not between the two ends of a range is an error, as is the empty set [] or [^]
//   \xHH         the byte HH (two hex digits), inside and outside sets
//   \\ \. \[ \] \^ \- \{ \}      that byte, inside and outside sets; any other \c is an error
//   {N}          after an atom: the atom N times in all, 1 <= N <= 4096, decimal digits only
//   any other byte is itself; outside a set ] { } must be escaped
// An expression of more than kClassExprMax classes is an error; the empty expression gives no classes.
// ignore_case adds the other ASCII case of every letter of a literal or a set, before the set is negated.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace bce {

constexpr size_t kClassExprMax = 4096;       // = BCE_HIP_CLASS_MAX_LEN

struct ClassExpr {
  const uint8_t *s;
  size_t len, at = 0;
  const char *why = nullptr;

  bool fail(const char *w) { why = w; return false; }
  static int hex(uint8_t c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }
  // the byte an escape names; at stands behind the backslash
  bool escape(uint32_t &c) {
    if (at >= len) return fail("a backslash at the end");
    const uint8_t e = s[at++];
    if (e == 'x') {
      if (at + 2 > len || hex(s[at]) < 0 || hex(s[at + 1]) < 0) return fail("\\x wants two hex digits");
      c = (uint32_t)(hex(s[at]) * 16 + hex(s[at + 1]));
      at += 2;
      return true;
    }
    if (e == '\\' || e == '.' || e == '[' || e == ']' || e == '^' || e == '-' || e == '{' || e == '}') { c = e; return true; }
    return fail("an escape that is not one of \\xHH \\\\ \\. \\[ \\] \\^ \\- \\{ \\}");
  }
  // one byte of a set: itself or an escape; at stands on it
  bool item(uint32_t &c) {
    c = s[at++];
    return c != '\\' || escape(c);
  }
  // a set; at stands behind the [
  bool set(uint32_t w[8]) {
    bool negate = false, any = false;
    if (at < len && s[at] == '^') { negate = true; ++at; }
    for (;;) {
      if (at >= len) return fail("a set without its ]");
      if (s[at] == ']') { ++at; break; }
      if (s[at] == '-') return fail("a - that is not inside a range (write \\-)");
      uint32_t a, b;
      if (!item(a)) return false;
      b = a;
      if (at < len && s[at] == '-') {
        ++at;
        if (at >= len) return fail("a set without its ]");
        if (s[at] == ']' || s[at] == '-') return fail("a - that is not inside a range (write \\-)");
        if (!item(b)) return false;
        if (a > b) return fail("a range whose first byte is above its last");
      }
      for (uint32_t c = a; c <= b; ++c) w[c >> 5] |= 1u << (c & 31u);
      any = true;
    }
    if (!any) return fail("an empty set");
    fold = true;
    neg = negate;
    return true;
  }
  bool fold = false, neg = false;              // of the atom just read: letters take their other case; the set is negated

  bool compile(bool ignore_case, std::vector<uint32_t> &masks) {
    masks.clear();
    bool atom = false;                         // the last thing read was an atom: {N} may follow
    while (at < len) {
      const uint8_t ch = s[at++];
      uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (ch == '{') {
        if (!atom) return fail("{ without an atom before it (write \\{)");
        uint32_t count = 0, digits = 0;
        while (at < len && s[at] >= '0' && s[at] <= '9' && digits < 8) { count = count * 10 + (uint32_t)(s[at++] - '0'); ++digits; }
        if (digits == 0 || at >= len || s[at] != '}') return fail("{N} wants decimal digits and its }");
        ++at;
        if (count < 1 || count > kClassExprMax) return fail("a repeat count outside 1 .. 4096");
        if (masks.size() / 8 + (count - 1) > kClassExprMax) return fail("more than 4096 classes");
        const size_t from = masks.size() - 8;
        for (uint32_t r = 1; r < count; ++r) for (size_t k = 0; k < 8; ++k) masks.push_back(masks[from + k]);
        atom = false;
        continue;
      }
      if (ch == ']' || ch == '}') return fail("] or } outside a set or a repeat (write \\] \\})");
      fold = neg = false;
      if (ch == '.') {
        for (uint32_t &v : w) v = 0xFFFFFFFFu;
      } else if (ch == '[') {
        if (!set(w)) return false;
      } else {
        uint32_t c = ch;
        if (ch == '\\' && !escape(c)) return false;
        w[c >> 5] |= 1u << (c & 31u);
        fold = true;
      }
      if (fold && ignore_case)
        for (uint32_t c = 'a'; c <= 'z'; ++c) {
          const uint32_t u = c - 32u;
          if (((w[c >> 5] >> (c & 31u)) | (w[u >> 5] >> (u & 31u))) & 1u) { w[c >> 5] |= 1u << (c & 31u); w[u >> 5] |= 1u << (u & 31u); }
        }
      if (neg) for (uint32_t &v : w) v = ~v;
      if (masks.size() / 8 >= kClassExprMax) return fail("more than 4096 classes");
      masks.insert(masks.end(), w, w + 8);
      atom = true;
    }
    return true;
  }
};

// masks: 8 words per class of expr[0, len).  False: the expression is malformed, *why (if given) says how; masks is then undefined.
inline bool compile_classes(const uint8_t *expr, size_t len, bool ignore_case, std::vector<uint32_t> &masks, const char **why = nullptr) {
  ClassExpr e{expr, len};
  const bool ok = e.compile(ignore_case, masks);
  if (why) *why = e.why;
  return ok;
}

}  // namespace bce
