// Stand-alone driver for the tokenizer of
// kuberay_amd/_native/json_decode.hpp (no Python). Built and run by
// tests/test_json_decode_sanitizers.py under -fsanitize=address,undefined.
// Every input is copied to a heap buffer of exactly its size first, so a
// read one byte past the end is an error the sanitizer reports. Exits 0 when
// every check holds; prints the failed check and exits 1 otherwise.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "json_decode.hpp"

using kuberay_json::Result;

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__,         \
                   __LINE__, #cond);                                      \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

// Writes the event sequence down as text: `{` `}` `[` `]`, k(key) s(string)
// i(int) d(double, %.17g) t f n, separated by spaces. Non-ASCII strings get
// a `*` after their letter.
struct Recorder {
  std::string out;
  int abort_after = -1;  // events to accept before returning false
  int seen = 0;

  bool ev(const std::string& s) {
    if (abort_after >= 0 && seen >= abort_after) return false;
    ++seen;
    if (!out.empty()) out.push_back(' ');
    out += s;
    return true;
  }
  bool begin_object() { return ev("{"); }
  bool end_object() { return ev("}"); }
  bool begin_array() { return ev("["); }
  bool end_array() { return ev("]"); }
  bool key(const char* p, size_t n, bool ascii, uint64_t h) {
    CHECK(h == kuberay_json::hash_bytes(p, n));
    return ev(std::string(ascii ? "k(" : "k*(") + std::string(p, n) + ")");
  }
  bool string(const char* p, size_t n, bool ascii) {
    for (size_t i = 0; i < n; ++i) {
      CHECK(!ascii || (static_cast<unsigned char>(p[i]) & 0x80) == 0);
    }
    return ev(std::string(ascii ? "s(" : "s*(") + std::string(p, n) + ")");
  }
  bool int64(int64_t v) {
    char buf[32];
    std::snprintf(buf, sizeof buf, "i(%" PRId64 ")", v);
    return ev(buf);
  }
  bool float64(double v) {
    char buf[48];
    std::snprintf(buf, sizeof buf, "d(%.17g)", v);
    return ev(buf);
  }
  bool boolean(bool v) { return ev(v ? "t" : "f"); }
  bool null() { return ev("n"); }
};

struct Parsed {
  Result result;
  std::string events;
};

static Parsed parse(const std::string& doc, int abort_after = -1) {
  std::unique_ptr<char[]> exact(new char[doc.size() ? doc.size() : 1]);
  std::memcpy(exact.get(), doc.data(), doc.size());
  Recorder rec;
  rec.abort_after = abort_after;
  kuberay_json::Tokenizer<Recorder> tok(rec);
  Parsed p;
  p.result = tok.document(exact.get(), doc.size());
  p.events = rec.out;
  return p;
}

static void expect_ok(const std::string& doc, const std::string& events) {
  Parsed p = parse(doc);
  if (p.result != Result::kOk || p.events != events) {
    std::fprintf(stderr, "document %s\n  result %d\n  events %s\n  wanted %s\n",
                 doc.c_str(), static_cast<int>(p.result), p.events.c_str(),
                 events.c_str());
    std::exit(1);
  }
}

static void expect(const std::string& doc, Result want) {
  Parsed p = parse(doc);
  if (p.result != want) {
    std::fprintf(stderr, "document %s: result %d, wanted %d\n", doc.c_str(),
                 static_cast<int>(p.result), static_cast<int>(want));
    std::exit(1);
  }
}

static void values() {
  expect_ok("{}", "{ }");
  expect_ok("[]", "[ ]");
  expect_ok("[[],{},[{}]]", "[ [ ] { } [ { } ] ]");
  expect_ok("{\"\":\"\"}", "{ k() s() }");
  expect_ok("{\"a\":[1,-2,true,false,null,\"x\"]}",
            "{ k(a) [ i(1) i(-2) t f n s(x) ] }");
  expect_ok(" { \"a\" : [ 1 , 2 ] , \"b\" : { } } ",
            "{ k(a) [ i(1) i(2) ] k(b) { } }");
  expect_ok("\"top\"", "s(top)");
  expect_ok("7", "i(7)");
  // the same key in different objects is no duplicate
  expect_ok("{\"a\":{\"a\":1},\"b\":{\"a\":2}}",
            "{ k(a) { k(a) i(1) } k(b) { k(a) i(2) } }");
  expect_ok("[{\"a\":1},{\"a\":2}]", "[ { k(a) i(1) } { k(a) i(2) } ]");
}

static void numbers() {
  expect_ok("[0,-0,9223372036854775807,-9223372036854775808]",
            "[ i(0) i(0) i(9223372036854775807) i(-9223372036854775808) ]");
  expect("9223372036854775808", Result::kUnsupported);
  expect("-9223372036854775809", Result::kUnsupported);
  expect("18446744073709551616", Result::kUnsupported);
  expect("123456789012345678901234567890", Result::kUnsupported);
  expect_ok("[0.1,1e-7,1E+22,5e-324,1.7976931348623157e308,-0.0,1.0,1e2]",
            "[ d(0.10000000000000001) d(9.9999999999999995e-08) d(1e+22) "
            "d(4.9406564584124654e-324) d(1.7976931348623157e+308) d(-0) "
            "d(1) d(100) ]");
  expect("1e999", Result::kUnsupported);   // inf in json.loads
  expect("1e-999", Result::kUnsupported);  // 0.0 in json.loads
  expect("NaN", Result::kUnsupported);
  expect("Infinity", Result::kUnsupported);
  expect("-Infinity", Result::kUnsupported);
  expect("[NaN]", Result::kUnsupported);
  for (const char* bad : {"01", "-", "+1", "1.", ".5", "1e", "1e+", "-a",
                          "0x10", "1.e3", "Nan", "Inf", "-Inf", "--1"}) {
    expect(bad, Result::kMalformed);
  }
}

static void strings() {
  expect_ok("\"\\\"\\\\\\/\\b\\f\\n\\r\\t\"", "s(\"\\/\b\f\n\r\t)");
  expect_ok("\"a\\u0041b\"", "s(aAb)");
  expect_ok("\"\\u00e9\"", "s*(\xC3\xA9)");
  expect_ok("\"\\u20AC\"", "s*(\xE2\x82\xAC)");
  expect_ok("\"\\ud83d\\ude00\"", "s*(\xF0\x9F\x98\x80)");
  expect_ok("\"caf\xC3\xA9 \xE2\x82\xAC \xF0\x9F\x98\x80\"",
            "s*(caf\xC3\xA9 \xE2\x82\xAC \xF0\x9F\x98\x80)");
  expect_ok("{\"k\\u00e9y\":1}", "{ k*(k\xC3\xA9y) i(1) }");
  // a long string takes the eight-bytes-at-a-time path, with the escape,
  // the high byte and the closing quote at every alignment
  for (int pad = 0; pad < 20; ++pad) {
    const std::string a(pad, 'x');
    expect_ok("\"" + a + "\\n" + a + "\"", "s(" + a + "\n" + a + ")");
    expect_ok("\"" + a + "\xC3\xA9" + a + "\"", "s*(" + a + "\xC3\xA9" + a + ")");
    expect_ok("[\"" + a + "\",1]", "[ s(" + a + ") i(1) ]");
    expect("\"" + a + "\x01" + a + "\"", Result::kMalformed);
    expect("\"" + a, Result::kMalformed);
  }
  {
    Parsed p = parse("\"a\\u0000b\"");
    CHECK(p.result == Result::kOk);
    CHECK(p.events == std::string("s(a\0b)", 6));
  }
  // lone surrogates: json.loads keeps them, this decoder does not
  expect("\"\\ud800\"", Result::kUnsupported);
  expect("\"\\udc00\"", Result::kUnsupported);
  expect("\"\\ud800x\"", Result::kUnsupported);
  expect("\"\\ud800\\u0041\"", Result::kUnsupported);
  expect("\"\\ud800\\n\"", Result::kUnsupported);
  expect("{\"\\udfff\":1}", Result::kUnsupported);
  // bad escapes
  for (const char* bad : {"\"\\x\"", "\"\\u12\"", "\"\\u12G4\"", "\"\\\"",
                          "\"\\u\"", "\"\\ud83d\\uZZZZ\"", "\"\\a\"", "\"\\'\"",
                          "\"\\U0041\""}) {
    expect(bad, Result::kMalformed);
  }
  // raw control characters and broken UTF-8
  expect(std::string("\"a\nb\""), Result::kMalformed);
  expect(std::string("\"a\0b\"", 5), Result::kMalformed);
  for (const char* bad : {"\"\x80\"", "\"\xC3\"", "\"\xC3(\"", "\"\xC0\xAF\"",
                          "\"\xE0\x80\xAF\"", "\"\xED\xA0\x80\"",
                          "\"\xF4\x90\x80\x80\"", "\"\xF8\x88\x80\x80\x80\"",
                          "\"\xE2\x82\"", "\"\xF0\x9F\x98\""}) {
    expect(bad, Result::kMalformed);
  }
}

static void structure() {
  for (const char* bad : {"", " ", "{", "}", "[", "]", "{\"a\"}", "{\"a\":}",
                          "{\"a\":1,}", "{,}", "[1,]", "[,1]", "[1 2]",
                          "{\"a\":1 \"b\":2}", "{a:1}", "{1:2}", "[1]]",
                          "{}{}", "{} x", "tru", "nul", "fals", "truex",
                          "[true false]", "{\"a\":1}}", "'a'"}) {
    expect(bad, Result::kMalformed);
  }
  // duplicate keys, spelled the same or not
  expect("{\"a\":1,\"a\":2}", Result::kUnsupported);
  expect("{\"a\":1,\"b\":2,\"\\u0061\":3}", Result::kUnsupported);
  expect("{\"\\u0061\":1,\"b\":2,\"a\":3}", Result::kUnsupported);
  expect("{\"x\":{\"k\":1,\"j\":2,\"k\":3}}", Result::kUnsupported);
  expect("{\"\":1,\"\":2}", Result::kUnsupported);
  // depth
  auto nest = [](int n, char open, char close) {
    return std::string(n, open) + std::string(n, close);
  };
  expect(nest(kuberay_json::kMaxDepth, '[', ']'), Result::kOk);
  expect(nest(kuberay_json::kMaxDepth + 1, '[', ']'), Result::kUnsupported);
  expect(nest(200, '[', ']'), Result::kUnsupported);
  std::string objs;
  for (int i = 0; i < 200; ++i) objs += "{\"a\":";
  objs += "1" + std::string(200, '}');
  expect(objs, Result::kUnsupported);
  expect(std::string(100000, '['), Result::kUnsupported);  // no deep recursion
}

// Every proper prefix of a document whose root is an object is not a
// document, and says so without reading past its end.
static void truncation() {
  const std::string doc =
      "{\"kind\":\"Pod\",\"n\":[1,-2.5e3,true,null],\"s\":\"a\\u00e9\\n"
      "\\ud83d\\ude00 long enough for the word path\",\"o\":{\"\":{}},"
      "\"u\":\"\xC3\xA9\xF0\x9F\x98\x80\"}";
  CHECK(parse(doc).result == Result::kOk);
  for (size_t n = 0; n < doc.size(); ++n) {
    const Result r = parse(doc.substr(0, n)).result;
    if (r != Result::kMalformed && r != Result::kUnsupported) {
      std::fprintf(stderr, "prefix of %zu bytes: result %d\n", n,
                   static_cast<int>(r));
      std::exit(1);
    }
  }
  // and a visitor may stop the walk at any event
  const int total = 40;
  for (int k = 0; k < total; ++k) {
    Parsed p = parse(doc, k);
    CHECK(p.result == Result::kAborted || p.result == Result::kOk);
    if (p.result == Result::kOk) break;
    CHECK(k + 1 < total);
  }
}

struct Entry {
  Result result;
  std::string events;
};

static Entry entry(const std::string* rest, const std::string* meta,
                   const std::string* status, bool whole) {
  Recorder rec;
  kuberay_json::Tokenizer<Recorder> tok(rec);
  Entry e;
  e.result = tok.entry(rest, meta, status, whole);
  e.events = rec.out;
  return e;
}

// The event sequence of a three-section object is that of the blob the
// store's assembler writes: rest members, then "metadata", then "status".
static void sections() {
  const std::string rest =
      "\"apiVersion\":\"v1\",\"kind\":\"Pod\",\"spec\":{\"containers\":[]}";
  const std::string meta = "{\"name\":\"p\",\"labels\":{\"a\":\"b\"}}";
  const std::string status = "{\"phase\":\"Running\"}";
  const std::string rest_events =
      "k(apiVersion) s(v1) k(kind) s(Pod) k(spec) { k(containers) [ ] }";
  const std::string meta_events =
      "k(metadata) { k(name) s(p) k(labels) { k(a) s(b) } }";
  const std::string status_events = "k(status) { k(phase) s(Running) }";

  Entry e = entry(&rest, &meta, &status, false);
  CHECK(e.result == Result::kOk);
  CHECK(e.events ==
        "{ " + rest_events + " " + meta_events + " " + status_events + " }");
  CHECK(parse("{" + rest + ",\"metadata\":" + meta + ",\"status\":" + status +
              "}").events == e.events);

  e = entry(&rest, nullptr, &status, false);
  CHECK(e.result == Result::kOk);
  CHECK(e.events == "{ " + rest_events + " " + status_events + " }");
  e = entry(nullptr, &meta, nullptr, false);
  CHECK(e.result == Result::kOk);
  CHECK(e.events == "{ " + meta_events + " }");
  const std::string empty;
  e = entry(&empty, &meta, &status, false);
  CHECK(e.result == Result::kOk);
  CHECK(e.events == "{ " + meta_events + " " + status_events + " }");
  e = entry(nullptr, nullptr, nullptr, false);
  CHECK(e.result == Result::kOk);
  CHECK(e.events == "{ }");

  // a whole entry is one document
  const std::string whole = "[1,{\"a\":null}]";
  e = entry(&whole, &meta, &status, true);
  CHECK(e.result == Result::kOk);
  CHECK(e.events == "[ i(1) { k(a) n } ]");

  // sections that are not what the assembler writes
  const std::string dup = "\"kind\":\"Pod\",\"metadata\":{}";
  CHECK(entry(&dup, &meta, nullptr, false).result == Result::kUnsupported);
  const std::string dup_status = "\"status\":1";
  CHECK(entry(&dup_status, nullptr, &status, false).result ==
        Result::kUnsupported);
  for (const char* bad : {"\"a\":1,", "\"a\":1}", "{\"a\":1}", "\"a\"", ",",
                          "\"a\":1 \"b\":2"}) {
    const std::string r = bad;
    CHECK(entry(&r, &meta, nullptr, false).result == Result::kMalformed);
  }
  for (const char* bad : {"", "{", "{}{}", "{} ,", "{\"a\":1"}) {
    const std::string m = bad;
    CHECK(entry(&rest, &m, nullptr, false).result == Result::kMalformed);
    CHECK(entry(&rest, &meta, &m, false).result == Result::kMalformed);
  }
  const std::string nan = "{\"x\":NaN}";
  CHECK(entry(&rest, &meta, &nan, false).result == Result::kUnsupported);
}

static void utf8_validator() {
  CHECK(kuberay_json::valid_utf8("", 0));
  CHECK(kuberay_json::valid_utf8("abc", 3));
  CHECK(kuberay_json::valid_utf8("\xC2\x80", 2));
  CHECK(kuberay_json::valid_utf8("\xEF\xBF\xBF", 3));
  CHECK(kuberay_json::valid_utf8("\xF4\x8F\xBF\xBF", 4));
  CHECK(!kuberay_json::valid_utf8("\xC1\xBF", 2));
  CHECK(!kuberay_json::valid_utf8("\xF5\x80\x80\x80", 4));
  CHECK(!kuberay_json::valid_utf8("\xF0\x8F\xBF\xBF", 4));
  CHECK(kuberay_json::hash_bytes("abcdefgh", 8) !=
        kuberay_json::hash_bytes("abcdefg", 7));
  CHECK(kuberay_json::hash_bytes("", 0) != kuberay_json::hash_bytes("\0", 1));
}

int main() {
  values();
  numbers();
  strings();
  structure();
  truncation();
  sections();
  utf8_validator();
  std::printf("json_decode_check OK\n");
  return 0;
}
