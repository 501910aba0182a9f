// Key comparator family and key normalization (host + device).
//
// Parity: src/Merger/CompareFunc.cc:29-113. The Java key class name selects one of three raw
// comparators over the *serialized* key bytes:
//   Text                               -> skip the VInt length prefix, memcmp, then length
//   Boolean/Byte/Short/Int/LongWritable-> memcmp of the raw bytes, then length
//   BytesWritable/ImmutableBytesWritable -> skip the 4-byte length, memcmp, then length
// Anything else is unsupported (the reference throws -> host falls back to vanilla shuffle).
//
// mapred.uda.key.order=hadoop (KeyOrder::kHadoop) replaces the memcmp of the numeric classes by Hadoop's
// own order and adds Float/Double/VInt/VLongWritable: each such key maps to one 64-bit word S whose
// unsigned order is the order of the class's Hadoop comparator (key_sortable). Text, the two bytes
// classes and BooleanWritable keep their comparators, which are byte compares in Hadoop as well.
//
// MI355X design: instead of calling the comparator O(log K) times per record from a heap, the GPU
// path normalizes every key once into a fixed-width big-endian prefix (`KeyNorm`) so almost all
// comparisons are two 64-bit integer compares; only prefix ties on keys longer than the prefix
// fall back to `key_compare` on the raw bytes.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "uda/vint.h"

namespace uda {

enum class KeyKind : int {
  kText = 0,
  kRaw = 1,
  kBytes = 2,
  // numeric kinds (KeyOrder::kHadoop only): ordered by key_sortable
  kByte = 3,
  kShort = 4,
  kInt = 5,
  kLong = 6,
  kVInt = 7,
  kVLong = 8,
  kFloat = 9,
  kDouble = 10,
  kUnsupported = -1
};

// mapred.uda.key.order: the reference's three comparators, or Hadoop's order for the numeric classes.
enum class KeyOrder : int { kReference = 0, kHadoop = 1 };
bool key_order_from_conf(const std::string& v, KeyOrder* out);
const char* key_order_name(KeyOrder o);

// Map a Java key class name to a comparator kind (CompareFunc.cc:95-113).
KeyKind key_kind_from_class(const char* java_class_name);
KeyKind key_kind_from_class(const char* java_class_name, KeyOrder order);
const char* key_kind_name(KeyKind k);

UDA_HD bool key_kind_numeric(KeyKind kind) { return (int)kind >= (int)KeyKind::kByte; }

// Key bytes a numeric kind with a fixed width requires; 0 for VInt / VLong and the byte kinds.
UDA_HD int key_fixed_bytes(KeyKind kind) {
  switch (kind) {
    case KeyKind::kByte: return 1;
    case KeyKind::kShort: return 2;
    case KeyKind::kInt:
    case KeyKind::kFloat: return 4;
    case KeyKind::kLong:
    case KeyKind::kDouble: return 8;
    default: return 0;
  }
}

// The sortable word of a numeric key: its unsigned order is the order of Hadoop's comparator of the class.
//   Byte/Short/Int/Long  exactly 1/2/4/8 bytes, big-endian two's complement v: S = v ^ 2^63
//   VInt/VLong           exactly the bytes its first byte announces (any encoding of a value is that value;
//                        under VInt the value lies in int): S = v ^ 2^63
//   Float/Double         4/8 bytes; Java's Float.compare / Double.compare: -0.0 < +0.0, every NaN is the one
//                        canonical NaN and the greatest; the float's word sits in the high 32 bits
// *ok = false (and 0) for a key of the wrong length.
UDA_HD uint64_t key_sortable(KeyKind kind, const uint8_t* key, int len, bool* ok) {
  constexpr uint64_t kSign = 1ull << 63;
  *ok = true;
  switch (kind) {
    case KeyKind::kByte:
    case KeyKind::kShort:
    case KeyKind::kInt:
    case KeyKind::kLong: {
      const int w = 1 << ((int)kind - (int)KeyKind::kByte);
      if (len != w) break;
      uint64_t u = 0;
      for (int i = 0; i < w; ++i) u = (u << 8) | key[i];
      const int sh = 64 - 8 * w;
      return (uint64_t)((int64_t)(u << sh) >> sh) ^ kSign;
    }
    case KeyKind::kVInt:
    case KeyKind::kVLong: {
      if (len < 1 || len != vint_decode_size((int)(int8_t)key[0])) break;
      int64_t v = 0;
      vint_decode(key, (size_t)len, &v);
      if (kind == KeyKind::kVInt && (v < INT32_MIN || v > INT32_MAX)) break;
      return (uint64_t)v ^ kSign;
    }
    case KeyKind::kFloat: {
      if (len != 4) break;
      uint32_t b = ((uint32_t)key[0] << 24) | ((uint32_t)key[1] << 16) | ((uint32_t)key[2] << 8) | key[3];
      if ((b & 0x7fffffffu) > 0x7f800000u) b = 0x7fc00000u;
      const uint32_t s = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
      return (uint64_t)s << 32;
    }
    case KeyKind::kDouble: {
      if (len != 8) break;
      uint64_t b = 0;
      for (int i = 0; i < 8; ++i) b = (b << 8) | key[i];
      if ((b & ~kSign) > 0x7ff0000000000000ull) b = 0x7ff8000000000000ull;
      return b ^ ((b >> 63) ? ~0ull : kSign);
    }
    default: break;
  }
  *ok = false;
  return 0;
}

constexpr int kBytesWritableLenBytes = 4;  // LENGTH_BYTES in the reference

// Offset of the comparable content inside the serialized key.
UDA_HD int key_content_offset(KeyKind kind, const uint8_t* key, int len) {
  if (kind == KeyKind::kText) {
    if (len <= 0) return 0;
    int s = vint_decode_size((int)(int8_t)key[0]);
    return s > len ? len : s;
  }
  if (kind == KeyKind::kBytes) return len < kBytesWritableLenBytes ? len : kBytesWritableLenBytes;
  return 0;
}

UDA_HD int bytes_compare(const uint8_t* a, int la, const uint8_t* b, int lb) {
  int n = la < lb ? la : lb;
  for (int i = 0; i < n; ++i) {
    if (a[i] != b[i]) return (int)a[i] - (int)b[i];
  }
  return la - lb;
}

// Full comparator on serialized keys. Sign matches the reference comparator.
// Numeric kinds compare their sortable words; a key of the wrong length sorts as the word 0 (the merge
// that meets one fails the task, see MergeQueue).
UDA_HD int key_compare(KeyKind kind, const uint8_t* a, int la, const uint8_t* b, int lb) {
  if (key_kind_numeric(kind)) {
    bool ok;
    const uint64_t sa = key_sortable(kind, a, la, &ok), sb = key_sortable(kind, b, lb, &ok);
    return sa < sb ? -1 : sa > sb ? 1 : 0;
  }
  int oa = key_content_offset(kind, a, la);
  int ob = key_content_offset(kind, b, lb);
  return bytes_compare(a + oa, la - oa, b + ob, lb - ob);
}

// Big-endian load of up to 8 bytes, zero padded on the right.
UDA_HD uint64_t load_be_prefix(const uint8_t* p, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint64_t v = 0;
  for (int i = 0; i < 8; ++i) v = (v << 8) | (uint64_t)(i < n ? p[i] : 0);
  return v;
#else
  // host: one unaligned load (or a short copy into a zeroed word) and a byte swap
  uint64_t w = 0;
  if (n >= 8)
    __builtin_memcpy(&w, p, 8);
  else if (n > 0)
    __builtin_memcpy(&w, p, (size_t)n);
  return __builtin_bswap64(w);
#endif
}

// Normalized key: the first 16 content bytes (big-endian, zero padded) and the content length.
// Order on (k0, k1) is consistent with memcmp on the content; when both contents are <= 16 bytes
// and (k0, k1) tie, the shorter content is smaller (the reference's `len1 - len2` tie-break).
struct KeyNorm {
  uint64_t k0;
  uint64_t k1;
  uint32_t len;  // content length (after skipping the VInt / 4-byte prefix)
  uint32_t off;  // content offset inside the serialized key
};

UDA_HD KeyNorm key_normalize(KeyKind kind, const uint8_t* key, int len) {
  KeyNorm n;
  if (key_kind_numeric(kind)) {  // the sortable word is the whole key: 8 content bytes, never a full compare
    bool ok;
    n.k0 = key_sortable(kind, key, len, &ok);
    n.k1 = 0;
    n.len = 8;
    n.off = 0;
    return n;
  }
  int o = key_content_offset(kind, key, len);
  int cl = len - o;
  n.k0 = load_be_prefix(key + o, cl);
  n.k1 = load_be_prefix(key + o + (cl > 8 ? 8 : cl), cl > 8 ? cl - 8 : 0);
  n.len = (uint32_t)cl;
  n.off = (uint32_t)o;
  return n;
}

// Compare two normalized keys. Returns <0, 0, >0; `needs_full` is set when the prefixes tie and
// at least one content is longer than 16 bytes (the caller must then run key_compare).
UDA_HD int keynorm_compare(const KeyNorm& a, const KeyNorm& b, bool* needs_full) {
  *needs_full = false;
  if (a.k0 != b.k0) return a.k0 < b.k0 ? -1 : 1;
  if (a.k1 != b.k1) return a.k1 < b.k1 ? -1 : 1;
  if (a.len <= 16 && b.len <= 16) return (int)a.len - (int)b.len;
  *needs_full = true;
  return 0;
}

// The Writable class a numeric kind stands for ("IntWritable"), for messages; and the failure of a task whose
// key has the wrong length: "... IntWritable key of 3 bytes (4 expected) in <where>". (Inline: the stand-alone
// programs of the engine link no other translation unit.)
inline const char* key_kind_class(KeyKind k) {
  switch (k) {
    case KeyKind::kByte: return "ByteWritable";
    case KeyKind::kShort: return "ShortWritable";
    case KeyKind::kInt: return "IntWritable";
    case KeyKind::kLong: return "LongWritable";
    case KeyKind::kVInt: return "VIntWritable";
    case KeyKind::kVLong: return "VLongWritable";
    case KeyKind::kFloat: return "FloatWritable";
    case KeyKind::kDouble: return "DoubleWritable";
    default: return "key";
  }
}

inline std::string key_bad_length_message(KeyKind k, int64_t len, const std::string& where) {
  std::string want;
  switch (k) {
    case KeyKind::kByte: want = "1 expected"; break;
    case KeyKind::kShort: want = "2 expected"; break;
    case KeyKind::kInt:
    case KeyKind::kFloat: want = "4 expected"; break;
    case KeyKind::kLong:
    case KeyKind::kDouble: want = "8 expected"; break;
    case KeyKind::kVInt: want = "the length its first byte announces and a value in int expected"; break;
    default: want = "the length its first byte announces expected"; break;
  }
  return std::string("mapred.uda.key.order=hadoop: ") + key_kind_class(k) + " key of " + std::to_string(len) + " bytes (" +
         want + ") in " + where;
}

}  // namespace uda
