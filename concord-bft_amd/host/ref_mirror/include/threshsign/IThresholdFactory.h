// Mirror of threshsign/include/threshsign/IThresholdFactory.h:25-54 (same virtual API): what
// Cryptosystem::createThresholdFactory returns (ThresholdSignaturesTypes.cpp:44-58) and
// generateNewPseudorandomKeys / generateNewKeyPair call (:60-91).
#pragma once

#include <memory>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "ThresholdSignaturesTypes.h"

class IThresholdVerifier;
class IThresholdSigner;
class IShareSecretKey;
class IShareVerificationKey;

class IThresholdFactory {
 public:
  virtual ~IThresholdFactory() {}
  // verifKeysStr is indexed from 1: entry 0 is a placeholder
  virtual IThresholdVerifier* newVerifier(ShareID reqSigners, ShareID totalSigners, const char* publicKeyStr,
                                          const std::vector<std::string>& verifKeysStr) const = 0;
  virtual IThresholdSigner* newSigner(ShareID id, const char* secretKeyStr) const = 0;
  // signers indexed from 1 (entry 0 is null); the caller deletes them and the verifier
  virtual std::tuple<std::vector<IThresholdSigner*>, IThresholdVerifier*> newRandomSigners(
      NumSharesType reqSigners, NumSharesType numSigners) const = 0;
  virtual std::pair<std::unique_ptr<IShareSecretKey>, std::unique_ptr<IShareVerificationKey>> newKeyPair() const = 0;
};
