// helib_amd_ckks.hpp -- EncryptedArrayCx (include/helib/EncryptedArray.h:1150-1330, src/EaCx.cpp) for the C++17
// host: CKKS slot vectors into ciphertexts and back, the slot maps on the device (hx_ckks_encode / hx_ckks_embed /
// hx_ckks_decode, include/helib_amd.h).  m a power of two, 16 <= m <= 2^17.  Slot order is PAlgebra's (ZmStar::ith_rep):
// slot s holds the value at zeta^-T[m/4-1-s].  EncryptedArrayCx::decrypt -- rawDecrypt plus noise against the
// Li-Micciancio attack (src/Ctxt.cpp:3051-3115) from NTL's PRG -- is not offered: only rawDecrypt.
// (A header of its own: host_session.cpp and the other headers do not call the slot entry points.)
#pragma once
#include <cmath>
#include <complex>
#include <cstring>
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

private:
  const ChainContext* cc;
  const Context* dev;
};

}  // namespace helib_amd
