// helib_amd_ckks.hpp -- EncryptedArrayCx (include/helib/EncryptedArray.h:1150-1330, src/EaCx.cpp) for the C++17
// host: CKKS slot vectors into ciphertexts and back, the slot maps on the device (hx_ckks_encode / hx_ckks_embed /
// hx_ckks_decode, include/helib_amd.h).  m a power of two, 16 <= m <= 2^17.  Slot order is PAlgebra's (ZmStar::ith_rep):
// slot s holds the value at zeta^-T[m/4-1-s].  EncryptedArrayCx::decrypt -- rawDecrypt plus noise against the
// Li-Micciancio attack (src/Ctxt.cpp:3051-3115) from NTL's PRG -- is not offered: only rawDecrypt.
// Between slots: rotate / shift (src/EaCx.cpp:142-236), totalSums / runningSums (src/EncryptedArray.cpp:695-735),
// extractRealPart / extractImPart (src/EaCx.cpp:419-447).  MatMul1DExec is offered in python only
// (helib_amd/linalg.py); its device call hx_mul_add_many is plain C ABI.
// (A header of its own: host_session.cpp and the other headers do not call the slot entry points.)
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <memory>
#include <vector>

#include "helib_amd_keys.hpp"

namespace helib_amd {

using cx_double = std::complex<double>;
using zzX = std::vector<long>;

class EncryptedArrayCx {
public:
  EncryptedArrayCx(const ChainContext& c, const Context& d) : cc(&c), dev(&d)
  {
    if (!c.ckks)
      throw LogicError("bad args to CKKS_canonicalEmbedding");   // src/norms.cpp:505
    if (c.m & (c.m - 1))
      throw InvalidArgument("CKKS scheme only supports m as a power of two.");   // src/PAlgebra.cpp:463-467
  }
  long size() const { return cc->m / 4; }

  // the factor of encode(zzX&, array, useThisSize, precision) (src/EaCx.cpp:324-349): encodeScalingFactor / size,
  // size = the largest |v| over all the vectors when not given (1 if that is 0)
  double factor(const std::vector<std::vector<cx_double>>& vs, double useThisSize = -1, long precision = -1) const
  {
    if (useThisSize < 0)
      for (auto& v : vs)
        for (auto& x : v)
          if (useThisSize < std::abs(x))
            useThisSize = std::abs(x);
    if (useThisSize <= 0)
      useThisSize = 1.0;
    return (double)cc->encodeScalingFactor(precision) / useThisSize;
  }

  // CKKS_embedInSlots of B vectors at `scaling` into a DoubleCRT over idx (evaluation form); coeffs (optional)
  // receives the B zzX back to back.  "overflow in encoding" is the reference's LogicError.
  DoubleCRT encodeBatch(const std::vector<std::vector<cx_double>>& vs, double scaling, const IndexSet& idx,
                        std::vector<long>* coeffs = nullptr) const
  {
    const int B = (int)vs.size();
    if (B < 1)
      throw InvalidArgument("EncryptedArrayCx: no vectors");
    size_t ns = 0;
    for (auto& v : vs)
      ns = std::max(ns, v.size());
    if ((long)ns > size())
      throw InvalidArgument("EncryptedArrayCx: more values than slots");
    std::vector<double> in((size_t)B * ns * 2, 0.0);   // missing values are 0
    for (int b = 0; b < B; b++)
      for (size_t i = 0; i < vs[(size_t)b].size(); i++) {
        in[((size_t)b * ns + i) * 2] = vs[(size_t)b][i].real();
        in[((size_t)b * ns + i) * 2 + 1] = vs[(size_t)b][i].imag();
      }
    DoubleCRT out(*dev, idx, B, DoubleCRT::Uninitialized{});
    std::vector<int64_t> cf(coeffs ? (size_t)B * cc->phim : 0);
    const int rc = hx_ckks_encode(dev->handle(), in.data(), B, (int)ns, scaling, out.handle(),
                                  coeffs ? cf.data() : nullptr);
    if (rc == HX_ERR_INVALID && std::strcmp(hx_last_error(), "overflow in encoding") == 0)
      throw LogicError("overflow in encoding");
    check(rc);
    if (coeffs)
      coeffs->assign(cf.begin(), cf.end());
    return out;
  }

  // EncryptedArrayCx::encode(zzX&, array, useThisSize, precision) -> the factor
  double encode(zzX& ptxt, const std::vector<cx_double>& array, double useThisSize = -1, long precision = -1) const
  {
    const double f = factor({array}, useThisSize, precision);
    encodeBatch({array}, f, IndexSet{}, &ptxt);
    return f;
  }
  // EncryptedArrayCx::decode (src/EaCx.cpp:385-395): canonicalEmbedding(ptxt) / scaling
  void decode(std::vector<cx_double>& array, const zzX& ptxt, double scaling) const
  {
    if (!(scaling > 0))
      throw InvalidArgument("Scaling must be positive to decode");
    std::vector<double> f((size_t)cc->phim, 0.0);
    for (size_t i = 0; i < ptxt.size() && i < f.size(); i++)
      f[i] = (double)ptxt[i];
    std::vector<double> out((size_t)size() * 2);
    check(hx_ckks_embed(dev->handle(), f.data(), 1, out.data()));
    array.resize((size_t)size());
    for (size_t i = 0; i < array.size(); i++)
      array[i] = cx_double(out[2 * i], out[2 * i + 1]) / scaling;
  }

  // EncryptedArrayCx::encrypt (include/helib/EncryptedArray.h:1252-1266): encode with the factor of encode(), then
  // CKKSencrypt with the caller's useThisSize as ptxtSize
  void encrypt(Ctxt& ctxt, SecKey& key, const std::vector<cx_double>& ptxt, double useThisSize = -1,
               long precision = -1) const
  {
    ctxt = encryptBatch(key, {ptxt}, useThisSize, precision);
  }
  // B vectors -> one batched Ctxt (one factor for the batch; PubKey's CKKSencryptBatch)
  Ctxt encryptBatch(SecKey& key, const std::vector<std::vector<cx_double>>& vs, double useThisSize = -1,
                    long precision = -1) const
  {
    const double f = factor(vs, useThisSize, precision);
    DoubleCRT enc = encodeBatch(vs, f, cc->ctxtPrimes);
    return key.CKKSencryptBatch(enc, useThisSize, f);
  }

  // EncryptedArrayCx::rawDecrypt (src/EaCx.cpp:62-86), complex and real (`project`) forms, of a batch-1 Ctxt
  void rawDecrypt(const Ctxt& ctxt, const SecKey& key, std::vector<cx_double>& ptxt) const
  {
    ptxt = rawDecryptBatch(ctxt, key).at(0);
  }
  void rawDecrypt(const Ctxt& ctxt, const SecKey& key, std::vector<double>& ptxt) const
  {
    std::vector<cx_double> v;
    rawDecrypt(ctxt, key, v);
    ptxt.resize(v.size());
    for (size_t i = 0; i < v.size(); i++)
      ptxt[i] = v[i].real();
  }
  // every element of a batched Ctxt: the inner product with the key, then hx_ckks_decode (value / ratFactor and
  // the embedding on the device, one download)
  std::vector<std::vector<cx_double>> rawDecryptBatch(const Ctxt& ctxt, const SecKey& key) const
  {
    std::unique_ptr<DoubleCRT> acc = key.innerProduct(ctxt);
    const int B = acc ? acc->batch() : 1;
    std::vector<double> out((size_t)B * size() * 2, 0.0);
    if (acc)
      check(hx_ckks_decode(acc->handle(), ctxt.lnRatFactor, out.data()));
    std::vector<std::vector<cx_double>> r((size_t)B, std::vector<cx_double>((size_t)size()));
    for (int b = 0; b < B; b++)
      for (long i = 0; i < size(); i++)
        r[(size_t)b][(size_t)i] = cx_double(out[((size_t)b * size() + i) * 2], out[((size_t)b * size() + i) * 2 + 1]);
    return r;
  }

  // ---- between slots ----
  // defaultErr / defaultScale (include/helib/EncryptedArray.h:1315-1349): neither depends on the data
  double defaultErr() const { return cc->noiseBoundForUniform(0.5, (double)cc->phim); }
  double defaultScale(double err, long prec = -1) const
  {
    if (err < 1.0)
      err = 1.0;
    const long r = prec < 0 ? cc->r : prec;
    int e;
    std::frexp(1 / err, &e);
    return std::ldexp(1.0, (int)(r - e + 1));
  }
  // EncryptedArrayCx::rotate = rotate1D(ctxt, 0, amt) (src/EaCx.cpp:142-164, 222-228): slot j moves to slot
  // (j + amt) mod size
  void rotate(Ctxt& ctxt, long amt) const
  {
    const long ord = size();
    amt %= ord;
    if (amt == 0)
      return;
    if (amt < 0)
      amt += ord;
    ctxt.smartAutomorph(zMStar().genToPow(0, amt));
  }
  // EncryptedArrayCx::shift = shift1D(ctxt, 0, k) (src/EaCx.cpp:166-221, 229-235): the encoded 0/1 mask first
  // (encode(EncodedPtxt&, ...), :238-278: mag = Norm(mask) = 1, the default scale and error), then the automorphism
  void shift(Ctxt& ctxt, long k) const
  {
    const long ord = size();
    if (k <= -ord || k >= ord) {
      ctxt.parts.clear();
      return;
    }
    long amt = k % ord;
    if (amt == 0)
      return;
    if (amt < 0)
      amt += ord;
    const long val = zMStar().genToPow(0, k < 0 ? amt - ord : amt);
    std::vector<cx_double> mask((size_t)ord);
    for (long j = 0; j < ord; j++)
      mask[(size_t)j] = (j + k >= ord || j + k < 0) ? 0.0 : 1.0;
    if (!ctxt.parts.empty()) {
      const double err = defaultErr(), scale = defaultScale(err);
      DoubleCRT enc = encodeBatch({mask}, scale, sorted(ctxt.primeSet));
      ctxt.multByConstantCKKS(enc, 1.0, scale, err);
    }
    ctxt.smartAutomorph(val);
  }
  // totalSums (src/EncryptedArray.cpp:707-735)
  void totalSums(Ctxt& ctxt) const
  {
    const long n = size();
    if (n == 1)
      return;
    const Ctxt orig = ctxt;
    long k = 0;
    while ((n >> k) != 0)
      k++;   // NTL::NumBits(n)
    long e = 1;
    for (long i = k - 2; i >= 0; i--) {
      Ctxt tmp1 = ctxt;
      rotate(tmp1, e);
      ctxt += tmp1;
      e = 2 * e;
      if ((n >> i) & 1) {
        Ctxt tmp2 = orig;
        rotate(tmp2, e);
        ctxt += tmp2;
        e += 1;
      }
    }
  }
  // runningSums (src/EncryptedArray.cpp:695-705)
  void runningSums(Ctxt& ctxt) const
  {
    const long n = size();
    for (long shamt = 1; shamt < n; shamt *= 2) {
      Ctxt tmp = ctxt;
      shift(tmp, shamt);
      ctxt += tmp;
    }
  }
  // src/EaCx.cpp:419-425: (c + conj(c)) * 0.5
  void extractRealPart(Ctxt& c) const
  {
    Ctxt tmp = c;
    tmp.complexConj();
    c += tmp;
    c.multByConstantCKKS(0.5);
  }
  // src/EaCx.cpp:432-447: (conj(c) - c) * i * 0.5, i encoded as encodei does (:368-372: size 1)
  void extractImPart(Ctxt& c) const
  {
    {
      Ctxt tmp = c;
      c.complexConj();
      c -= tmp;
    }
    if (c.parts.empty())
      return;
    const std::vector<cx_double> vi((size_t)size(), cx_double(0.0, 1.0));
    const double f = factor({vi}, 1.0);
    DoubleCRT enc = encodeBatch({vi}, f, sorted(c.primeSet));
    c.multByConstantCKKS(enc, 1.0, f, cc->encodeRoundingError());
    c.multByConstantCKKS(0.5);
  }

private:
  template <class S>
  static IndexSet sorted(const S& s)
  {
    IndexSet v(s.begin(), s.end());
    std::sort(v.begin(), v.end());
    return v;
  }
  const ZmStar& zMStar() const
  {
    if (!zm)
      zm = std::make_shared<ZmStar>(cc->m, -1);
    return *zm;
  }
  const ChainContext* cc;
  const Context* dev;
  mutable std::shared_ptr<ZmStar> zm;
};

}  // namespace helib_amd
