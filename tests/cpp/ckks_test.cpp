// EncryptedArrayCx in C++ (include/helib_amd_ckks.hpp) on the device:
//   ckks_test <m> <bits> <B> <out.bin>
// encryptBatch of two batches of B vectors, multiplyBy, rawDecryptBatch: the product slot by slot within the
// ciphertext's errorBound; the decoded product (B x m/4 complex doubles) goes to out.bin for the python class to
// compare against, with the bound on stdout.  Also: encode/decode of a zzX, encrypt / rawDecrypt (both forms),
// CKKSencryptBatch at B = 1 equal word for word to CKKSencrypt from the same seed, "overflow in encoding".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "helib_amd_ckks.hpp"

using namespace helib_amd;

#define REQUIRE(c)                                                   \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                      \
    }                                                                \
  } while (0)

// the inputs tests/test_ckks_slots_gpu.py builds the same way
static std::vector<std::vector<cx_double>> vectors(long n, int B, double s)
{
  std::vector<std::vector<cx_double>> v((size_t)B, std::vector<cx_double>((size_t)n));
  for (int b = 0; b < B; b++)
    for (long i = 0; i < n; i++)
      v[(size_t)b][(size_t)i] = cx_double(0.5 * std::cos(s * (double)i + 1.1 * b), 0.5 * std::sin(0.23 * (double)i + s * b));
  return v;
}

int main(int argc, char** argv)
{
  if (argc < 5)
    return 2;
  const long m = atol(argv[1]), bits = atol(argv[2]);
  const int B = atoi(argv[3]);
  try {
    ChainContext cc(m, -1, 20, bits, 3, 3.2, 10.0, 0, 3, 0, true);
    auto dev = cc.makeDeviceContext(0);
    SecKey sk(cc, *dev, 31);
    sk.GenSecKey(2);
    EncryptedArrayCx ea(cc, *dev);
    REQUIRE(ea.size() == m / 4);
    const auto a = vectors(ea.size(), B, 0.37), b = vectors(ea.size(), B, 0.61);

    Ctxt ca = ea.encryptBatch(sk, a), cb = ea.encryptBatch(sk, b);
    ca.multiplyBy(cb);
    const auto got = ea.rawDecryptBatch(ca, sk);
    const double bound = std::exp(ca.lnNoise - ca.lnRatFactor);   // Ctxt::errorBound
    REQUIRE((int)got.size() == B);
    double err = 0;
    std::vector<double> flat;
    for (int k = 0; k < B; k++)
      for (long i = 0; i < ea.size(); i++) {
        const cx_double g = got[(size_t)k][(size_t)i];
        err = std::max(err, std::abs(g - a[(size_t)k][(size_t)i] * b[(size_t)k][(size_t)i]));
        flat.push_back(g.real());
        flat.push_back(g.imag());
      }
    REQUIRE(err <= bound);
    FILE* f = fopen(argv[4], "wb");
    REQUIRE(f && fwrite(flat.data(), sizeof(double), flat.size(), f) == flat.size());
    fclose(f);

    // encode / decode of one zzX (src/EaCx.cpp:324-349, 385-395)
    zzX z;
    const double fac = ea.encode(z, a[0]);
    REQUIRE((long)z.size() == cc.phim);
    std::vector<cx_double> back;
    ea.decode(back, z, fac);
    double d = 0;
    for (long i = 0; i < ea.size(); i++)
      d = std::max(d, std::abs(back[(size_t)i] - a[0][(size_t)i]));
    REQUIRE(d <= cc.encodeRoundingError() / fac);

    // encrypt / rawDecrypt, complex and real forms
    Ctxt one = ea.encryptBatch(sk, {a[0]});
    ea.encrypt(one, sk, b[0]);
    std::vector<cx_double> vc;
    std::vector<double> vr;
    ea.rawDecrypt(one, sk, vc);
    ea.rawDecrypt(one, sk, vr);
    const double b1 = std::exp(one.lnNoise - one.lnRatFactor);
    for (long i = 0; i < ea.size(); i++) {
      REQUIRE(std::abs(vc[(size_t)i] - b[0][(size_t)i]) <= b1);
      REQUIRE(vr[(size_t)i] == vc[(size_t)i].real());
    }

    // CKKSencryptBatch at B = 1 is CKKSencrypt, word for word, from the same seed
    SecKey s1(cc, *dev, 4242), s2(cc, *dev, 4242);
    s1.GenSecKey(2);
    s2.GenSecKey(2);
    const double f1 = ea.factor({a[0]});
    DoubleCRT enc = ea.encodeBatch({a[0]}, f1, cc.ctxtPrimes);
    Ctxt c1 = s1.CKKSencrypt(enc, 1.0, f1), c2 = s2.CKKSencryptBatch(enc, 1.0, f1);
    REQUIRE(c1.lnRatFactor == c2.lnRatFactor && c1.lnNoise == c2.lnNoise && c1.ptxtMag == c2.ptxtMag);
    REQUIRE(c1.parts.size() == c2.parts.size());
    for (auto& kv : c1.parts)
      REQUIRE(kv.second.getRows() == c2.parts.at(kv.first).getRows());
    // ... and the integer-polynomial CKKSencrypt of the same zzX, from the same seed again
    SecKey s3(cc, *dev, 4242);
    s3.GenSecKey(2);
    zzX z1;
    ea.encodeBatch({a[0]}, f1, IndexSet{}, &z1);
    Ctxt c3 = s3.CKKSencrypt(z1, 1.0, f1);
    for (auto& kv : c1.parts)
      REQUIRE(kv.second.getRows() == c3.parts.at(kv.first).getRows());

    // CKKS_embedInSlots: "overflow in encoding" (LogicError)
    bool threw = false;
    try {
      ea.encodeBatch({a[0]}, 1e30, cc.ctxtPrimes);
    } catch (const LogicError& e) {
      threw = std::strcmp(e.what(), "overflow in encoding") == 0;
    }
    REQUIRE(threw);
    printf("errorBound %.17g\n", bound);
    printf("ckks_test OK (max slot error %.3e)\n", err);
  } catch (const std::exception& e) {
    fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
  return 0;
}
