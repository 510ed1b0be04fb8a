// Slot rotations, sums and parts of EncryptedArrayCx in C++ (include/helib_amd_ckks.hpp) and hx_mul_add_many called
// directly, on the device:
//   linalg_test <m> <bits> <B> <out.bin>
// Every decrypted result is within the ciphertext's errorBound of the plaintext map; the rotation by one of the
// batch (B x m/4 complex doubles) goes to out.bin for the python class to compare against, its bound to stdout.
// hx_mul_add_many: 300 terms, two parts, constants on more primes than the outputs, against the
// { tmp = b; tmp *= a; x += tmp } sequence word for word; its error returns (no terms, a null entry).
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

typedef std::vector<cx_double> Vec;

// the inputs tests/test_ckks_linalg_cpp_gpu.py builds the same way
static std::vector<Vec> vectors(long n, int B, double s)
{
  std::vector<Vec> v((size_t)B, Vec((size_t)n));
  for (int b = 0; b < B; b++)
    for (long i = 0; i < n; i++)
      v[(size_t)b][(size_t)i] = cx_double(0.5 * std::cos(s * (double)i + 1.1 * b), 0.5 * std::sin(0.23 * (double)i + s * b));
  return v;
}
// the plaintext maps (src/EncryptedArray.cpp:887-963, 1974-2007)
static Vec p_rotate(const Vec& v, long k)
{
  const long n = (long)v.size();
  Vec t((size_t)n);
  for (long i = 0; i < n; i++)
    t[(size_t)(((i + k) % n + n) % n)] = v[(size_t)i];
  return t;
}
static Vec p_shift(Vec v, long k)
{
  const long n = (long)v.size();
  for (long j = 0; j < n; j++)
    if (j + k >= n || j + k < 0)
      v[(size_t)j] = 0;
  return p_rotate(v, k);
}

static double worst(const std::vector<Vec>& got, const std::vector<Vec>& want)
{
  double e = 0;
  for (size_t b = 0; b < want.size(); b++)
    for (size_t i = 0; i < want[b].size(); i++)
      e = std::max(e, std::abs(got[b][i] - want[b][i]));
  return e;
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
    ZmStar z(m, -1);
    std::vector<long> strategy;
    add1DMatrices(sk, z, strategy);
    if (!sk.haveKeySWmatrix(1, m - 1))
      sk.GenKeySWmatrix(1, m - 1);
    sk.setKeySwitchMap();
    EncryptedArrayCx ea(cc, *dev);
    const long n = ea.size();
    const auto a = vectors(n, B, 0.37);

    auto run = [&](const char* what, auto op, auto map, std::vector<Vec>* keep, double* keep_bound) -> int {
      Ctxt ct = ea.encryptBatch(sk, a);
      op(ct);
      std::vector<Vec> want;
      for (auto& v : a)
        want.push_back(map(v));
      const auto got = ea.rawDecryptBatch(ct, sk);
      const double bound = std::exp(ct.lnNoise - ct.lnRatFactor), err = worst(got, want);
      printf("%s: max slot error %.3e, errorBound %.3e\n", what, err, bound);
      if (keep) {
        *keep = got;
        *keep_bound = bound;
      }
      return err <= bound ? 0 : 1;
    };
    std::vector<Vec> rot1;
    double rot1_bound = 0;
    REQUIRE(!run("rotate 1", [&](Ctxt& c) { ea.rotate(c, 1); }, [&](const Vec& v) { return p_rotate(v, 1); }, &rot1, &rot1_bound));
    REQUIRE(!run("rotate -3", [&](Ctxt& c) { ea.rotate(c, -3); }, [&](const Vec& v) { return p_rotate(v, -3); }, nullptr, nullptr));
    REQUIRE(!run("rotate n+5", [&](Ctxt& c) { ea.rotate(c, n + 5); }, [&](const Vec& v) { return p_rotate(v, n + 5); }, nullptr, nullptr));
    REQUIRE(!run("shift 2", [&](Ctxt& c) { ea.shift(c, 2); }, [&](const Vec& v) { return p_shift(v, 2); }, nullptr, nullptr));
    REQUIRE(!run("shift -7", [&](Ctxt& c) { ea.shift(c, -7); }, [&](const Vec& v) { return p_shift(v, -7); }, nullptr, nullptr));
    {
      Ctxt ct = ea.encryptBatch(sk, a);
      ea.shift(ct, n);
      REQUIRE(ct.parts.empty());
      ct = ea.encryptBatch(sk, a);
      ea.shift(ct, -n);
      REQUIRE(ct.parts.empty());
    }
    REQUIRE(!run("totalSums", [&](Ctxt& c) { ea.totalSums(c); },
                 [&](const Vec& v) {
                   cx_double s = 0;
                   for (auto& x : v)
                     s += x;
                   return Vec(v.size(), s);
                 },
                 nullptr, nullptr));
    REQUIRE(!run("runningSums", [&](Ctxt& c) { ea.runningSums(c); },
                 [&](Vec v) {
                   for (size_t i = 1; i < v.size(); i++)
                     v[i] += v[i - 1];
                   return v;
                 },
                 nullptr, nullptr));
    REQUIRE(!run("extractRealPart", [&](Ctxt& c) { ea.extractRealPart(c); },
                 [&](Vec v) {
                   for (auto& x : v)
                     x = x.real();
                   return v;
                 },
                 nullptr, nullptr));
    REQUIRE(!run("extractImPart", [&](Ctxt& c) { ea.extractImPart(c); },
                 [&](Vec v) {
                   for (auto& x : v)
                     x = x.imag();
                   return v;
                 },
                 nullptr, nullptr));
    std::vector<double> flat;
    for (auto& v : rot1)
      for (auto& x : v) {
        flat.push_back(x.real());
        flat.push_back(x.imag());
      }
    FILE* f = fopen(argv[4], "wb");
    REQUIRE(f && fwrite(flat.data(), sizeof(double), flat.size(), f) == flat.size());
    fclose(f);

    // hx_mul_add_many against the sequence it replaces
    {
      const int T = 300;
      const IndexSet all = cc.ctxtPrimes;
      const IndexSet own(all.begin(), all.begin() + (all.size() > 2 ? 2 : 1));
      uint8_t key[32];
      for (int i = 0; i < 32; i++)
        key[i] = (uint8_t)(7 * i + 1);
      std::vector<DoubleCRT> cs, i0, i1;
      for (int t = 0; t < T; t++) {
        cs.emplace_back(*dev, all, 1, DoubleCRT::Uninitialized{});
        cs.back().randomize(key, 10 + (uint64_t)t);
        i0.emplace_back(*dev, own, B, DoubleCRT::Uninitialized{});
        i0.back().randomize(key, 1000 + (uint64_t)t);
        i1.emplace_back(*dev, own, B, DoubleCRT::Uninitialized{});
        i1.back().randomize(key, 2000 + (uint64_t)t);
      }
      DoubleCRT o0(*dev, own, B, DoubleCRT::Uninitialized{}), o1(*dev, own, B, DoubleCRT::Uninitialized{});
      o0.randomize(key, 1);
      o1.randomize(key, 2);
      DoubleCRT w0 = o0, w1 = o1;
      for (int t = 0; t < T; t++) {
        DoubleCRT t0 = i0[(size_t)t], t1 = i1[(size_t)t];
        t0 *= cs[(size_t)t];
        t1 *= cs[(size_t)t];
        w0 += t0;
        w1 += t1;
      }
      std::vector<const hx_poly*> pc, p0, p1;
      for (int t = 0; t < T; t++) {
        pc.push_back(cs[(size_t)t].handle());
        p0.push_back(i0[(size_t)t].handle());
        p1.push_back(i1[(size_t)t].handle());
      }
      check(hx_mul_add_many(o0.handle(), o1.handle(), pc.data(), p0.data(), p1.data(), T, 1));
      REQUIRE(o0.getRows() == w0.getRows() && o1.getRows() == w1.getRows());
      // one part, overwriting
      DoubleCRT x(*dev, own, B), wx(*dev, own, B);
      for (int t = 0; t < 7; t++) {
        DoubleCRT t0 = i0[(size_t)t];
        t0 *= cs[(size_t)t];
        wx += t0;
      }
      x.randomize(key, 3);
      check(hx_mul_add_many(x.handle(), nullptr, pc.data(), p0.data(), nullptr, 7, 0));
      REQUIRE(x.getRows() == wx.getRows());
      // the error returns
      REQUIRE(hx_mul_add_many(x.handle(), nullptr, pc.data(), p0.data(), nullptr, 0, 0) == HX_ERR_INVALID);
      std::vector<const hx_poly*> holes = p0;
      holes[3] = nullptr;
      REQUIRE(hx_mul_add_many(x.handle(), nullptr, pc.data(), holes.data(), nullptr, 7, 0) == HX_ERR_INVALID);
      REQUIRE(hx_mul_add_many(nullptr, nullptr, pc.data(), p0.data(), nullptr, 7, 0) == HX_ERR_INVALID);
      REQUIRE(hx_mul_add_many(x.handle(), o1.handle(), pc.data(), p0.data(), nullptr, 7, 0) == HX_ERR_INVALID);
      REQUIRE(x.getRows() == wx.getRows());   // a refused call writes nothing
    }
    printf("errorBound %.17g\n", rot1_bound);
    printf("linalg_test OK\n");
  } catch (const std::exception& e) {
    fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
  return 0;
}
