// json_decode — stored JSON sections straight to a Python object tree.
//
// A read used to assemble an entry's three sections (store_core.hpp) into one
// bytes object and hand it to json.loads, which re-creates every key, "True",
// label value and image name of every pod on every parse. The decoder here
// walks the sections where they lie and builds the same tree: no blob, no
// whole-object str, and the short strings that repeat from object to object
// come out of a small table instead of being created again.
//
// Two halves:
//   Tokenizer — plain C++17, no Python. Walks JSON bytes and drives a visitor
//               (begin/end object, begin/end array, key, string, int64,
//               double, true/false/null). tests/native/json_decode_check.cpp
//               drives it alone, under sanitizers.
//   TreeBuilder — a visitor that builds dict / list / str / int / float /
//               bool / None. Compiled only where KUBERAY_JSON_WITH_PYTHON is
//               defined (engine.cpp).
//
// The contract is "what json.loads gives, or nothing". Whatever the tokenizer
// would not reproduce exactly it reports as kUnsupported (as opposed to
// kMalformed) and the caller takes the blob + json.loads path for that
// object: integers outside int64, NaN / Infinity / -Infinity, lone
// surrogates, a key that occurs twice in one object, nesting deeper than
// kMaxDepth, and floats std::from_chars calls out of range (json.loads gives
// inf or 0.0 there). Every other float is the token's correctly rounded
// double, which is what CPython's parser gives.
#pragma once

#include <charconv>
#include <cstdint>
#include <cstring>
#include <list>
#include <string>
#include <system_error>
#include <vector>

namespace kuberay_json {

enum class Result {
  kOk,
  kMalformed,    // not JSON (json.loads raises)
  kUnsupported,  // JSON, but not reproduced here: take the json.loads path
  kAborted,      // the visitor returned false
};

// Containers nested deeper than this are unsupported (the native encoder
// declines at the same depth, so such trees are stored as whole blobs).
constexpr int kMaxDepth = 128;

// Hash of a byte string by 8-byte words; the dedupe of an object's keys and
// the builder's string table both use it. Equal bytes give equal hashes and
// nothing more is asked of it: every hit is confirmed by memcmp.
inline uint64_t hash_bytes(const char* p, size_t n) {
  constexpr uint64_t k = 0x9E3779B97F4A7C15ull;
  uint64_t h = (n + 1) * k;
  while (n >= 8) {
    uint64_t w;
    std::memcpy(&w, p, 8);
    h = (h ^ w) * k;
    h ^= h >> 29;
    p += 8;
    n -= 8;
  }
  if (n) {
    uint64_t w = 0;
    std::memcpy(&w, p, n);
    h = (h ^ w) * k;
    h ^= h >> 29;
  }
  return h;
}

// Strict UTF-8: no overlong forms, no surrogates, nothing past U+10FFFF.
inline bool valid_utf8(const char* s, size_t n) {
  const unsigned char* p = reinterpret_cast<const unsigned char*>(s);
  const unsigned char* end = p + n;
  while (p < end) {
    const unsigned c = *p;
    if (c < 0x80) { ++p; continue; }
    size_t need;
    unsigned lo = 0x80, hi = 0xBF;
    if (c >= 0xC2 && c <= 0xDF) need = 1;
    else if (c == 0xE0) { need = 2; lo = 0xA0; }
    else if (c == 0xED) { need = 2; hi = 0x9F; }
    else if (c >= 0xE1 && c <= 0xEF) need = 2;
    else if (c == 0xF0) { need = 3; lo = 0x90; }
    else if (c >= 0xF1 && c <= 0xF3) need = 3;
    else if (c == 0xF4) { need = 3; hi = 0x8F; }
    else return false;
    if (static_cast<size_t>(end - p) <= need) return false;
    if (p[1] < lo || p[1] > hi) return false;
    for (size_t i = 2; i <= need; ++i) {
      if (p[i] < 0x80 || p[i] > 0xBF) return false;
    }
    p += need + 1;
  }
  return true;
}

// Visitor: every method returns bool, false aborts the walk.
//   begin_object() end_object() begin_array() end_array()
//   key(p, n, ascii, hash)   string(p, n, ascii)
//   int64(v) float64(v) boolean(v) null()
// Keys and strings arrive unescaped, as valid UTF-8 (`ascii`: no byte has
// its high bit set); the bytes are only good for the length of the call.
// A Tokenizer is good for one walk (document() or entry(), once): a walk that
// ends early leaves its bookkeeping of open objects behind.
template <class V>
class Tokenizer {
 public:
  explicit Tokenizer(V& v) : v_(v) {
    keys_.reserve(64);
    frames_.reserve(16);
  }

  // One complete document.
  Result document(const char* p, size_t n) {
    const char* end = p + n;
    Result r = value(p, end, 0);
    if (r != Result::kOk) return r;
    skip_ws(p, end);
    return p == end ? Result::kOk : Result::kMalformed;
  }

  // One stored entry, the way Blob::write lays it out: `rest` holds the
  // members `"k":v,"k":v` without braces, `meta` and `status` the values of
  // "metadata" and "status"; any of the three may be null. With `whole`,
  // `rest` is a complete document and the others are ignored.
  Result entry(const std::string* rest, const std::string* meta,
               const std::string* status, bool whole) {
    if (whole) {
      if (rest == nullptr) return Result::kMalformed;
      return document(rest->data(), rest->size());
    }
    if (!v_.begin_object()) return Result::kAborted;
    frames_.push_back(keys_.size());
    if (rest != nullptr && !rest->empty()) {
      const char* p = rest->data();
      const char* end = p + rest->size();
      Result r = members(p, end, 1);
      if (r != Result::kOk) return r;
      skip_ws(p, end);
      if (p != end) return Result::kMalformed;
    }
    if (meta != nullptr) {
      Result r = section("metadata", 8, *meta);
      if (r != Result::kOk) return r;
    }
    if (status != nullptr) {
      Result r = section("status", 6, *status);
      if (r != Result::kOk) return r;
    }
    keys_.resize(frames_.back());
    frames_.pop_back();
    return v_.end_object() ? Result::kOk : Result::kAborted;
  }

 private:
  struct KeyRec {
    uint64_t hash;
    const char* p;
    size_t n;
  };

  static void skip_ws(const char*& p, const char* end) {
    while (p < end && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) ++p;
  }

  Result section(const char* name, size_t name_len, const std::string& body) {
    const uint64_t h = hash_bytes(name, name_len);
    if (!note_key(h, name, name_len, false)) return Result::kUnsupported;
    if (!v_.key(name, name_len, true, h)) return Result::kAborted;
    const char* p = body.data();
    const char* end = p + body.size();
    Result r = value(p, end, 1);
    if (r != Result::kOk) return r;
    skip_ws(p, end);
    return p == end ? Result::kOk : Result::kMalformed;
  }

  // Records a key of the innermost object; false when that object already
  // has it. `copy`: the bytes live in scratch and must be kept.
  bool note_key(uint64_t h, const char* p, size_t n, bool copy) {
    for (size_t i = frames_.back(); i < keys_.size(); ++i) {
      const KeyRec& k = keys_[i];
      if (k.hash == h && k.n == n && std::memcmp(k.p, p, n) == 0) return false;
    }
    if (copy) {
      escaped_keys_.emplace_back(p, n);
      p = escaped_keys_.back().data();
    }
    keys_.push_back(KeyRec{h, p, n});
    return true;
  }

  // `"k":v` pairs separated by commas, at least one; stops after the last
  // value (the caller checks what follows).
  Result members(const char*& p, const char* end, int depth) {
    for (;;) {
      skip_ws(p, end);
      if (p == end || *p != '"') return Result::kMalformed;
      const char* s;
      size_t n;
      bool ascii, escaped;
      Result r = scan_string(p, end, s, n, ascii, escaped);
      if (r != Result::kOk) return r;
      const uint64_t h = hash_bytes(s, n);
      if (!note_key(h, s, n, escaped)) return Result::kUnsupported;
      if (!v_.key(s, n, ascii, h)) return Result::kAborted;
      skip_ws(p, end);
      if (p == end || *p != ':') return Result::kMalformed;
      ++p;
      r = value(p, end, depth);
      if (r != Result::kOk) return r;
      skip_ws(p, end);
      if (p == end || *p != ',') return Result::kOk;
      ++p;
    }
  }

  Result value(const char*& p, const char* end, int depth) {
    skip_ws(p, end);
    if (p == end) return Result::kMalformed;
    switch (*p) {
      case '{': {
        if (depth >= kMaxDepth) return Result::kUnsupported;
        ++p;
        if (!v_.begin_object()) return Result::kAborted;
        skip_ws(p, end);
        if (p == end) return Result::kMalformed;
        if (*p == '}') {
          ++p;
          return v_.end_object() ? Result::kOk : Result::kAborted;
        }
        frames_.push_back(keys_.size());
        Result r = members(p, end, depth + 1);
        if (r != Result::kOk) return r;
        if (p == end || *p != '}') return Result::kMalformed;
        ++p;
        keys_.resize(frames_.back());
        frames_.pop_back();
        return v_.end_object() ? Result::kOk : Result::kAborted;
      }
      case '[': {
        if (depth >= kMaxDepth) return Result::kUnsupported;
        ++p;
        if (!v_.begin_array()) return Result::kAborted;
        skip_ws(p, end);
        if (p == end) return Result::kMalformed;
        if (*p == ']') {
          ++p;
          return v_.end_array() ? Result::kOk : Result::kAborted;
        }
        for (;;) {
          Result r = value(p, end, depth + 1);
          if (r != Result::kOk) return r;
          skip_ws(p, end);
          if (p == end) return Result::kMalformed;
          if (*p == ',') { ++p; continue; }
          if (*p == ']') { ++p; break; }
          return Result::kMalformed;
        }
        return v_.end_array() ? Result::kOk : Result::kAborted;
      }
      case '"': {
        const char* s;
        size_t n;
        bool ascii, escaped;
        Result r = scan_string(p, end, s, n, ascii, escaped);
        if (r != Result::kOk) return r;
        return v_.string(s, n, ascii) ? Result::kOk : Result::kAborted;
      }
      case 't':
        if (!literal(p, end, "true", 4)) return Result::kMalformed;
        return v_.boolean(true) ? Result::kOk : Result::kAborted;
      case 'f':
        if (!literal(p, end, "false", 5)) return Result::kMalformed;
        return v_.boolean(false) ? Result::kOk : Result::kAborted;
      case 'n':
        if (!literal(p, end, "null", 4)) return Result::kMalformed;
        return v_.null() ? Result::kOk : Result::kAborted;
      case 'N':
        return literal(p, end, "NaN", 3) ? Result::kUnsupported
                                         : Result::kMalformed;
      case 'I':
        return literal(p, end, "Infinity", 8) ? Result::kUnsupported
                                              : Result::kMalformed;
      default:
        return number(p, end);
    }
  }

  static bool literal(const char*& p, const char* end, const char* lit,
                      size_t n) {
    if (static_cast<size_t>(end - p) < n || std::memcmp(p, lit, n) != 0) {
      return false;
    }
    p += n;
    return true;
  }

  static bool is_digit(char c) { return c >= '0' && c <= '9'; }

  // -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][-+]?[0-9]+)? — json.loads' grammar. A
  // token without fraction and exponent is an int there, everything else a
  // float.
  Result number(const char*& p, const char* end) {
    const char* start = p;
    bool neg = false;
    if (*p == '-') {
      neg = true;
      ++p;
      if (p == end) return Result::kMalformed;
      if (*p == 'I') {
        return literal(p, end, "Infinity", 8) ? Result::kUnsupported
                                              : Result::kMalformed;
      }
    }
    if (!is_digit(*p)) return Result::kMalformed;
    const char* digits = p;
    uint64_t mag = 0;
    if (*p == '0') {
      ++p;
    } else {
      while (p < end && is_digit(*p)) {
        // past 19 digits the value is outside int64 whatever `mag` says
        if (p - digits < 19) mag = mag * 10 + static_cast<uint64_t>(*p - '0');
        ++p;
      }
    }
    const size_t ndigits = static_cast<size_t>(p - digits);
    bool is_float = false;
    if (p < end && *p == '.') {
      ++p;
      if (p == end || !is_digit(*p)) return Result::kMalformed;
      while (p < end && is_digit(*p)) ++p;
      is_float = true;
    }
    if (p < end && (*p == 'e' || *p == 'E')) {
      ++p;
      if (p < end && (*p == '+' || *p == '-')) ++p;
      if (p == end || !is_digit(*p)) return Result::kMalformed;
      while (p < end && is_digit(*p)) ++p;
      is_float = true;
    }
    if (!is_float) {
      constexpr uint64_t kMax = 0x7FFFFFFFFFFFFFFFull;
      if (ndigits > 19 || mag > kMax + (neg ? 1 : 0)) return Result::kUnsupported;
      // -(2^63) is reached without overflow: negate in uint64, then convert
      const int64_t v = static_cast<int64_t>(neg ? (0 - mag) : mag);
      return v_.int64(v) ? Result::kOk : Result::kAborted;
    }
    double d = 0.0;
    const std::from_chars_result fc =
        std::from_chars(start, p, d, std::chars_format::general);
    // out of range is inf or 0.0 in json.loads; anything short of the whole
    // token cannot happen for this grammar, and is not trusted if it does
    if (fc.ec != std::errc() || fc.ptr != p) return Result::kUnsupported;
    return v_.float64(d) ? Result::kOk : Result::kAborted;
  }

  static int hex4(const char* p) {
    int v = 0;
    for (int i = 0; i < 4; ++i) {
      const char c = p[i];
      int d;
      if (c >= '0' && c <= '9') d = c - '0';
      else if (c >= 'a' && c <= 'f') d = c - 'a' + 10;
      else if (c >= 'A' && c <= 'F') d = c - 'A' + 10;
      else return -1;
      v = v * 16 + d;
    }
    return v;
  }

  void append_utf8(unsigned cp) {
    if (cp < 0x80) {
      scratch_.push_back(static_cast<char>(cp));
    } else if (cp < 0x800) {
      scratch_.push_back(static_cast<char>(0xC0 | (cp >> 6)));
      scratch_.push_back(static_cast<char>(0x80 | (cp & 0x3F)));
    } else if (cp < 0x10000) {
      scratch_.push_back(static_cast<char>(0xE0 | (cp >> 12)));
      scratch_.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3F)));
      scratch_.push_back(static_cast<char>(0x80 | (cp & 0x3F)));
    } else {
      scratch_.push_back(static_cast<char>(0xF0 | (cp >> 18)));
      scratch_.push_back(static_cast<char>(0x80 | ((cp >> 12) & 0x3F)));
      scratch_.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3F)));
      scratch_.push_back(static_cast<char>(0x80 | (cp & 0x3F)));
    }
  }

  // `p` at the opening quote; leaves it past the closing one. Without
  // escapes [s, s+n) points into the input, with them into scratch_.
  Result scan_string(const char*& p, const char* end, const char*& s,
                     size_t& n, bool& ascii, bool& escaped) {
    ++p;
    const char* run = p;
    unsigned char high = 0;
    escaped = false;
    for (;;) {
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__
      // Eight bytes at a time while none of them is a quote, a backslash or
      // a control character. The three tests can flag a byte above the first
      // real match but never one below it, so the lowest flag is exact.
      while (end - p >= 8) {
        constexpr uint64_t ones = 0x0101010101010101ull;
        constexpr uint64_t tops = 0x8080808080808080ull;
        uint64_t w;
        std::memcpy(&w, p, 8);
        const uint64_t q = w ^ (ones * '"'), b = w ^ (ones * '\\');
        const uint64_t m = (((q - ones) & ~q) | ((b - ones) & ~b) |
                            ((w - ones * 0x20) & ~w)) & tops;
        if (m == 0) {
          high |= static_cast<unsigned char>((w & tops) != 0 ? 0x80 : 0);
          p += 8;
          continue;
        }
        const unsigned skip = static_cast<unsigned>(__builtin_ctzll(m)) >> 3;
        if (skip) {
          const uint64_t before = w & ((1ull << (8 * skip)) - 1);
          high |= static_cast<unsigned char>((before & tops) != 0 ? 0x80 : 0);
          p += skip;
        }
        break;
      }
#endif
      if (p == end) return Result::kMalformed;
      const unsigned char c = static_cast<unsigned char>(*p);
      if (c == '"') break;
      if (c < 0x20) return Result::kMalformed;
      if (c != '\\') {
        high |= c;
        ++p;
        continue;
      }
      if (!escaped) {
        escaped = true;
        scratch_.clear();
      }
      scratch_.append(run, p - run);
      ++p;
      if (p == end) return Result::kMalformed;
      const char e = *p++;
      switch (e) {
        case '"': scratch_.push_back('"'); break;
        case '\\': scratch_.push_back('\\'); break;
        case '/': scratch_.push_back('/'); break;
        case 'b': scratch_.push_back('\b'); break;
        case 'f': scratch_.push_back('\f'); break;
        case 'n': scratch_.push_back('\n'); break;
        case 'r': scratch_.push_back('\r'); break;
        case 't': scratch_.push_back('\t'); break;
        case 'u': {
          if (end - p < 4) return Result::kMalformed;
          int cp = hex4(p);
          if (cp < 0) return Result::kMalformed;
          p += 4;
          if (cp >= 0xDC00 && cp <= 0xDFFF) return Result::kUnsupported;
          if (cp >= 0xD800 && cp <= 0xDBFF) {
            // json.loads pairs it only with an escaped low surrogate right
            // behind it; alone it stays a lone surrogate
            if (end - p < 6 || p[0] != '\\' || p[1] != 'u') {
              return Result::kUnsupported;
            }
            const int lo = hex4(p + 2);
            if (lo < 0) return Result::kMalformed;
            if (lo < 0xDC00 || lo > 0xDFFF) return Result::kUnsupported;
            p += 6;
            cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
          }
          if (cp >= 0x80) high |= 0x80;
          append_utf8(static_cast<unsigned>(cp));
          break;
        }
        default:
          return Result::kMalformed;
      }
      run = p;
    }
    if (escaped) {
      scratch_.append(run, p - run);
      s = scratch_.data();
      n = scratch_.size();
    } else {
      s = run;
      n = static_cast<size_t>(p - run);
    }
    ++p;
    ascii = (high & 0x80) == 0;
    if (!ascii && !valid_utf8(s, n)) return Result::kMalformed;
    return Result::kOk;
  }

  V& v_;
  std::string scratch_;
  std::vector<KeyRec> keys_;       // keys of the objects now open
  std::vector<size_t> frames_;     // where each open object's keys start
  std::list<std::string> escaped_keys_;   // storage for keys from scratch_
};

}  // namespace kuberay_json

#ifdef KUBERAY_JSON_WITH_PYTHON
#include <Python.h>

namespace kuberay_json {

// Keys, and string values up to kInternValueMax bytes, are looked up here
// before they are created: direct-mapped by hash_bytes, one strong reference
// per slot, a newcomer replaces what it collides with. ASCII only (the
// str's own bytes are then what is compared). At most kInternSlots short
// strings are held, so its memory is bounded (a few hundred KB when full).
// Guarded by the GIL.
constexpr size_t kInternSlots = 4096;
constexpr size_t kInternKeyMax = 64;
constexpr size_t kInternValueMax = 32;

struct InternSlot {
  uint64_t hash = 0;
  PyObject* str = nullptr;
};

inline InternSlot* intern_table() {
  static InternSlot table[kInternSlots];
  return table;
}

// New reference; nullptr with a Python error set.
inline PyObject* interned_ascii(const char* p, size_t n, uint64_t h) {
  InternSlot& slot = intern_table()[(h >> 20) & (kInternSlots - 1)];
  if (slot.str != nullptr && slot.hash == h &&
      static_cast<size_t>(PyUnicode_GET_LENGTH(slot.str)) == n &&
      std::memcmp(PyUnicode_1BYTE_DATA(slot.str), p, n) == 0) {
    Py_INCREF(slot.str);
    return slot.str;
  }
  PyObject* s = PyUnicode_New(static_cast<Py_ssize_t>(n), 127);
  if (s == nullptr) return nullptr;
  std::memcpy(PyUnicode_1BYTE_DATA(s), p, n);
  Py_INCREF(s);
  PyObject* old = slot.str;
  slot.str = s;
  slot.hash = h;
  Py_XDECREF(old);
  return s;
}

inline PyObject* make_str(const char* p, size_t n, bool ascii) {
  if (ascii) {
    PyObject* s = PyUnicode_New(static_cast<Py_ssize_t>(n), 127);
    if (s != nullptr) std::memcpy(PyUnicode_1BYTE_DATA(s), p, n);
    return s;
  }
  return PyUnicode_DecodeUTF8(p, static_cast<Py_ssize_t>(n), nullptr);
}

// The visitor that builds the tree. Containers are always new; strings may
// be shared with earlier results. A Python error (out of memory) aborts the
// walk; the caller clears it and falls back.
class TreeBuilder {
 public:
  TreeBuilder() = default;
  TreeBuilder(const TreeBuilder&) = delete;
  TreeBuilder& operator=(const TreeBuilder&) = delete;
  ~TreeBuilder() {
    for (int i = 0; i < depth_; ++i) {
      Py_XDECREF(stack_[i].container);
      Py_XDECREF(stack_[i].key);
    }
    Py_XDECREF(root_);
  }

  // The finished tree (new reference), once.
  PyObject* release() {
    PyObject* r = root_;
    root_ = nullptr;
    return r;
  }

  bool begin_object() { return push(PyDict_New()); }
  bool begin_array() { return push(PyList_New(0)); }
  bool end_object() { return pop(); }
  bool end_array() { return pop(); }

  bool key(const char* p, size_t n, bool ascii, uint64_t h) {
    PyObject* k = (ascii && n <= kInternKeyMax) ? interned_ascii(p, n, h)
                                                : make_str(p, n, ascii);
    if (k == nullptr) return false;
    stack_[depth_ - 1].key = k;
    return true;
  }

  bool string(const char* p, size_t n, bool ascii) {
    if (ascii && n <= kInternValueMax) {
      return add(interned_ascii(p, n, hash_bytes(p, n)));
    }
    return add(make_str(p, n, ascii));
  }

  bool int64(int64_t v) { return add(PyLong_FromLongLong(v)); }
  bool float64(double v) { return add(PyFloat_FromDouble(v)); }
  bool boolean(bool v) { return add(PyBool_FromLong(v)); }
  bool null() {
    Py_INCREF(Py_None);
    return add(Py_None);
  }

 private:
  struct Frame {
    PyObject* container = nullptr;
    PyObject* key = nullptr;  // the dict key waiting for its value
  };

  bool push(PyObject* c) {
    if (c == nullptr) return false;
    if (depth_ >= kMaxDepth + 1) {  // the tokenizer stops earlier
      Py_DECREF(c);
      return false;
    }
    stack_[depth_].container = c;
    stack_[depth_].key = nullptr;
    ++depth_;
    return true;
  }

  bool pop() {
    --depth_;
    PyObject* c = stack_[depth_].container;
    stack_[depth_].container = nullptr;
    return add(c);
  }

  // Steals `v` (nullptr: a Python error is set).
  bool add(PyObject* v) {
    if (v == nullptr) return false;
    if (depth_ == 0) {
      Py_XDECREF(root_);
      root_ = v;
      return true;
    }
    Frame& f = stack_[depth_ - 1];
    int rc;
    if (f.key != nullptr) {
      rc = PyDict_SetItem(f.container, f.key, v);
      Py_CLEAR(f.key);
    } else {
      rc = PyList_Append(f.container, v);
    }
    Py_DECREF(v);
    return rc == 0;
  }

  Frame stack_[kMaxDepth + 1];
  int depth_ = 0;
  PyObject* root_ = nullptr;
};

}  // namespace kuberay_json
#endif  // KUBERAY_JSON_WITH_PYTHON
