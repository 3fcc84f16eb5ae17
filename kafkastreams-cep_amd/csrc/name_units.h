// name_units.h — a JSON string's raw text (between the quotes, as the decoders' name spans
// give it) read as the UTF-16 code units of the Java String deserialize() builds: ASCII, the JSON
// escapes (\" \\ \/ \b \f \n \r \t \uXXXX) and well-formed UTF-8 (1-4 bytes, no surrogates, no overlong
// forms).  A header of its own so that code beside the [symbol] keying (symbol.hip) can read names
// the same way, on the device or the host (CEP_HD).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CEP_HD __host__ __device__
#else
#define CEP_HD
#endif

namespace cep {

// UTF-16 code units of a JSON string's raw text (between the quotes), one at a time
struct NameUnits {
  const uint8_t* p;
  uint32_t n, i = 0;
  uint32_t low = 0;  // pending low surrogate of a 4-byte UTF-8 sequence
  CEP_HD NameUnits(const uint8_t* s, uint32_t len) : p(s), n(len) {}
  CEP_HD static int hex(uint8_t c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
  }
  // next unit (0..0xFFFF), -1 at the end, -2 on malformed input
  CEP_HD int next() {
    if (low) {
      const int u = (int)low;
      low = 0;
      return u;
    }
    if (i >= n) return -1;
    const uint8_t c = p[i];
    if (c == '\\') {
      if (i + 1 >= n) return -2;
      const uint8_t e = p[i + 1];
      i += 2;
      switch (e) {
        case '"': return '"';
        case '\\': return '\\';
        case '/': return '/';
        case 'b': return 8;
        case 'f': return 12;
        case 'n': return 10;
        case 'r': return 13;
        case 't': return 9;
        case 'u': {
          if (i + 4 > n) return -2;
          int v = 0;
          for (int k = 0; k < 4; k++) {
            const int h = hex(p[i + k]);
            if (h < 0) return -2;
            v = v * 16 + h;
          }
          i += 4;
          return v;
        }
        default: return -2;  // (the scanner throws on these: such records have a status)
      }
    }
    if (c < 0x80) {
      i++;
      return c;
    }
    // well-formed UTF-8 only
    int len = c >= 0xF0 && c <= 0xF4 ? 4 : c >= 0xE0 ? (c <= 0xEF ? 3 : 0) : c >= 0xC2 ? 2 : 0;
    if (!len || i + len > n) return -2;
    uint32_t cp = c & (len == 2 ? 0x1F : len == 3 ? 0x0F : 0x07);
    for (int k = 1; k < len; k++) {
      const uint8_t b = p[i + k];
      if ((b & 0xC0) != 0x80) return -2;
      cp = (cp << 6) | (b & 0x3F);
    }
    if ((len == 3 && (cp < 0x800 || (cp >= 0xD800 && cp <= 0xDFFF))) || (len == 4 && (cp < 0x10000 || cp > 0x10FFFF)))
      return -2;
    i += len;
    if (cp >= 0x10000) {
      cp -= 0x10000;
      low = 0xDC00 + (cp & 0x3FF);
      return (int)(0xD800 + (cp >> 10));
    }
    return (int)cp;
  }
};

}  // namespace cep
