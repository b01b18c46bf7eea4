// Strict DER front end of the ECDSA verifiers that take OpenSSL-style signatures (host only, no
// OpenSSL dependency): SEQUENCE { INTEGER r, INTEGER s } -> r || s, each left-padded to the
// order's width, as the batch ABI takes them.
//
// Accepted is exactly what OpenSSL 3.0.2's ECDSA_verify lets through before it looks at the
// curve: it parses with d2i_ECDSA_SIG, re-encodes with i2d_ECDSA_SIG and requires the same bytes
// and no trailing ones, so only the canonical encoding passes: definite lengths in their shortest
// form, integers with their shortest padding.  A negative INTEGER re-encodes to itself there and is
// then refused by the range check 1 <= r, s; here it is refused at once, as is an integer wider
// than the order (both are verdict false either way).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ecdsa_der_detail {
// a definite length in its shortest form at der[*pos]; advances *pos past it
inline bool length(const uint8_t* der, size_t len, size_t* pos, size_t* out) {
  if (*pos >= len) return false;
  const uint8_t l0 = der[(*pos)++];
  if (l0 < 0x80) {
    *out = l0;
    return true;
  }
  const size_t nb = l0 & 0x7F;
  if (nb == 0 || nb > 4 || len - *pos < nb) return false;  // indefinite (BER), oversized, cut short
  if (der[*pos] == 0) return false;                         // a leading zero byte: not the shortest form
  size_t v = 0;
  for (size_t i = 0; i < nb; i++) v = (v << 8) | der[(*pos)++];
  if (v < 0x80) return false;  // the short form would have done
  *out = v;
  return true;
}
// a non-negative INTEGER with its shortest padding -> out[0 .. width), big-endian, left-padded
inline bool integer(const uint8_t* der, size_t len, size_t* pos, size_t width, uint8_t* out) {
  if (*pos >= len || der[(*pos)++] != 0x02) return false;
  size_t n;
  if (!length(der, len, pos, &n)) return false;
  if (n == 0 || len - *pos < n) return false;
  const uint8_t* b = der + *pos;
  *pos += n;
  if (b[0] & 0x80) return false;                             // negative
  if (n > 1 && b[0] == 0 && !(b[1] & 0x80)) return false;    // a zero byte that no sign bit asks for
  if (b[0] == 0) {  // the sign byte (or the value 0 itself)
    b++;
    n--;
  }
  if (n > width) return false;  // wider than the order
  for (size_t i = 0; i < width - n; i++) out[i] = 0;
  for (size_t i = 0; i < n; i++) out[width - n + i] = b[i];
  return true;
}
}  // namespace ecdsa_der_detail

// out_rs: 2 * order_bytes bytes.  false: not a canonical DER ECDSA signature over an order of that
// width (out_rs unspecified); the verdict is then false.
inline bool ecdsa_der_to_rs(const uint8_t* der, size_t len, size_t order_bytes, uint8_t* out_rs) {
  using namespace ecdsa_der_detail;
  if (!der || len < 2 || der[0] != 0x30) return false;
  size_t pos = 1, body;
  if (!length(der, len, &pos, &body)) return false;
  if (len - pos != body) return false;  // cut short, or trailing bytes
  if (!integer(der, len, &pos, order_bytes, out_rs)) return false;
  if (!integer(der, len, &pos, order_bytes, out_rs + order_bytes)) return false;
  return pos == len;  // nothing after s inside the SEQUENCE
}

// The writer: r || s (each order_bytes wide, big-endian) -> the canonical SEQUENCE { INTEGER r,
// INTEGER s } that ecdsa_der_to_rs accepts (what i2d_ECDSA_SIG writes): shortest lengths, and a
// leading 00 only when the value's top bit is set (the value 0 is the single byte 00).
// out: at least ECDSA_DER_MAX_BYTES(order_bytes) bytes; *out_len = bytes written.
#define ECDSA_DER_MAX_BYTES(order_bytes) (2 * ((order_bytes) + 1 + 5) + 6)
namespace ecdsa_der_detail {
inline size_t put_length(uint8_t* out, size_t n) {
  if (n < 0x80) {
    out[0] = (uint8_t)n;
    return 1;
  }
  size_t nb = 0;
  for (size_t v = n; v; v >>= 8) nb++;
  out[0] = (uint8_t)(0x80 | nb);
  for (size_t i = 0; i < nb; i++) out[1 + i] = (uint8_t)(n >> (8 * (nb - 1 - i)));
  return 1 + nb;
}
// the INTEGER's content length: the value without leading zero bytes (one byte at least), plus the sign byte
inline size_t integer_bytes(const uint8_t* v, size_t width, size_t* skip) {
  size_t z = 0;
  while (z + 1 < width && v[z] == 0) z++;
  *skip = z;
  return (width - z) + ((v[z] & 0x80) ? 1 : 0);
}
inline size_t put_integer(uint8_t* out, const uint8_t* v, size_t width) {
  size_t skip;
  const size_t n = integer_bytes(v, width, &skip);
  size_t pos = 0;
  out[pos++] = 0x02;
  pos += put_length(out + pos, n);
  if (v[skip] & 0x80) out[pos++] = 0x00;
  for (size_t i = skip; i < width; i++) out[pos++] = v[i];
  return pos;
}
}  // namespace ecdsa_der_detail

inline bool ecdsa_rs_to_der(const uint8_t* rs, size_t order_bytes, uint8_t* out, size_t* out_len) {
  using namespace ecdsa_der_detail;
  if (!rs || !out || !out_len || order_bytes == 0) return false;
  uint8_t lenbuf[1 + sizeof(size_t)];
  size_t skip;
  const size_t nr = integer_bytes(rs, order_bytes, &skip), ns = integer_bytes(rs + order_bytes, order_bytes, &skip);
  const size_t body = (1 + put_length(lenbuf, nr) + nr) + (1 + put_length(lenbuf, ns) + ns);
  size_t pos = 0;
  out[pos++] = 0x30;
  pos += put_length(out + pos, body);
  pos += put_integer(out + pos, rs, order_bytes);
  pos += put_integer(out + pos, rs + order_bytes, order_bytes);
  *out_len = pos;
  return true;
}
