# Build of libcbft_hipcrypto (gfx950) and of the CPU oracle used by the tests.
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
CSRC    := concord-bft_amd/csrc
LIB     := concord-bft_amd/libcbft_hipcrypto.so
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Iinclude -I$(CSRC) -Wall -Wno-unused-function
ORACLE_LIB := oracle/libcbft_oracle.so
# The row-parallel field code (bn254_row.h, fe25519_row.h: row_shr / row_shl moves with zero fill) is built
# without LLVM's DPP combiner: on this toolchain (ROCm 7.2 LLVM, gfx950) folding those moves into
# their consumers left non-zero values in lanes that must read 0 (a G2 addition came out wrong in
# one inlined copy and right in another; tools/microbench/g2r_dbg2.hip reproduces it, and the
# host SIMD emulation of the same source is exact).  Costs one v_mov_dpp per move.
ROWFLAGS := -mllvm -amdgpu-dpp-combine=false

.PHONY: all lib oracle clean shim fe_row_shim bls_sign_shim bls_combine_shim bls_keygen_shim sha512_shim ecdsa_shim ecdsa_sign_shim ecdsa_p256_shim ecdsa_p256_sign_shim host_util_test sanitize selftest
all: lib oracle cpu host shim fe_row_shim bls_sign_shim bls_combine_shim bls_keygen_shim sha512_shim ecdsa_shim ecdsa_sign_shim ecdsa_p256_shim ecdsa_p256_sign_shim host_util_test selftest

lib: $(LIB)

$(CSRC)/ed25519_verify.o: $(CSRC)/ed25519_verify.hip $(CSRC)/*.h
	$(HIPCC) $(HIPFLAGS) $(ROWFLAGS) -c $< -o $@

# what every front end (cbft_*.cpp) compiles in through cbft_internal.h
INTERNAL_DEPS := $(CSRC)/cbft_internal.h $(CSRC)/cbft_host_util.h include/cbft_hipcrypto.h $(CSRC)/ed25519_sign.h $(CSRC)/ed25519_verify.h $(CSRC)/rsa_sign.h $(CSRC)/rsa_verify.h
$(CSRC)/cbft_hipcrypto.o: $(CSRC)/cbft_hipcrypto.cpp $(INTERNAL_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

BLS_DEPS := $(CSRC)/bls_kernels.h $(CSRC)/bls_common.h $(CSRC)/bn254_*.h $(CSRC)/row_lanes.h $(CSRC)/bls_ops.h $(CSRC)/sha256.h $(CSRC)/bls_glv.h
$(CSRC)/bls_kernels.o: $(CSRC)/bls_kernels.hip $(BLS_DEPS)
	$(HIPCC) $(HIPFLAGS) $(ROWFLAGS) -c $< -o $@

$(CSRC)/bls_pairing.o: $(CSRC)/bls_pairing.hip $(BLS_DEPS)
	$(HIPCC) $(HIPFLAGS) $(ROWFLAGS) -c $< -o $@

$(CSRC)/bls_msm_row.o: $(CSRC)/bls_msm_row.hip $(BLS_DEPS) $(CSRC)/bls_glv.h
	$(HIPCC) $(HIPFLAGS) $(ROWFLAGS) -c $< -o $@

$(CSRC)/bls_keys.o: $(CSRC)/bls_keys.hip $(CSRC)/bls_g2_shared.h $(BLS_DEPS)
	$(HIPCC) $(HIPFLAGS) $(ROWFLAGS) -c $< -o $@

$(CSRC)/rsa_verify.o: $(CSRC)/rsa_verify.hip $(CSRC)/rsa_verify.h $(CSRC)/sha256.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# Ed25519 signing: its own object (constant-time kernels; the verify kernels are not touched)
$(CSRC)/ed25519_sign.o: $(CSRC)/ed25519_sign.hip $(CSRC)/ed25519_sign.h $(CSRC)/ge25519.h $(CSRC)/fe25519*.h $(CSRC)/sc25519.h $(CSRC)/sha512.h $(CSRC)/safegcd30.h $(CSRC)/row_lanes.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/cbft_ed25519_sign.o: $(CSRC)/cbft_ed25519_sign.cpp $(INTERNAL_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# RSA signing: its own object (constant-time CRT kernels; rsa_verify.hip is not touched)
$(CSRC)/rsa_sign.o: $(CSRC)/rsa_sign.hip $(CSRC)/rsa_sign.h $(CSRC)/sha256.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/cbft_rsa_sign.o: $(CSRC)/cbft_rsa_sign.cpp $(INTERNAL_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/cbft_rsa.o: $(CSRC)/cbft_rsa.cpp $(INTERNAL_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# BLS share signing in batches: its own object (constant-time lane code; the other BLS kernels are not touched)
$(CSRC)/bls_sign_batch.o: $(CSRC)/bls_sign_batch.hip $(CSRC)/bls_sign_batch.h $(BLS_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/cbft_bls_sign.o: $(CSRC)/cbft_bls_sign.cpp $(INTERNAL_DEPS) $(CSRC)/bls_keygen_batch.h $(CSRC)/bls_sign_batch.h $(BLS_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# BLS verification in batches over many messages: its own objects (the other BLS kernels are not touched)
$(CSRC)/bls_verify_batch.o: $(CSRC)/bls_verify_batch.hip $(CSRC)/bls_verify_batch.h $(CSRC)/bls_sign_batch.h $(BLS_DEPS)
	$(HIPCC) $(HIPFLAGS) $(ROWFLAGS) -c $< -o $@

$(CSRC)/cbft_bls_verify_batch.o: $(CSRC)/cbft_bls_verify_batch.cpp $(INTERNAL_DEPS) $(CSRC)/bls_verify_batch.h $(CSRC)/bls_kernels.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# BLS share combination in batches over many certificates: its own objects (the other BLS kernels are not touched)
BLS_COMBINE_DEPS := $(CSRC)/bls_combine_batch.h $(CSRC)/bls_sign_batch.h $(BLS_DEPS)
$(CSRC)/bls_combine_batch.o: $(CSRC)/bls_combine_batch.hip $(BLS_COMBINE_DEPS)
	$(HIPCC) $(HIPFLAGS) $(ROWFLAGS) -c $< -o $@

$(CSRC)/cbft_bls_combine_batch.o: $(CSRC)/cbft_bls_combine_batch.cpp $(INTERNAL_DEPS) $(BLS_COMBINE_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# BLS multisig verification in batches over many signer sets: its own objects (the other BLS kernels are not touched)
BLS_MULTISIG_DEPS := $(CSRC)/bls_multisig_batch.h $(CSRC)/bls_verify_batch.h $(CSRC)/bls_g2_shared.h $(BLS_DEPS)
$(CSRC)/bls_multisig_batch.o: $(CSRC)/bls_multisig_batch.hip $(BLS_MULTISIG_DEPS)
	$(HIPCC) $(HIPFLAGS) $(ROWFLAGS) -c $< -o $@

$(CSRC)/cbft_bls_multisig_batch.o: $(CSRC)/cbft_bls_multisig_batch.cpp $(INTERNAL_DEPS) $(BLS_MULTISIG_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# BLS key derivation and dealing in batches: its own objects (constant-time lane code; the other BLS kernels are not touched)
BLS_KEYGEN_DEPS := $(CSRC)/bls_keygen_batch.h $(CSRC)/bls_sign_batch.h $(BLS_DEPS)
$(CSRC)/bls_keygen_batch.o: $(CSRC)/bls_keygen_batch.hip $(BLS_KEYGEN_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/cbft_bls_keygen.o: $(CSRC)/cbft_bls_keygen.cpp $(INTERNAL_DEPS) $(BLS_KEYGEN_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# ECDSA secp256k1 verification: its own objects (no other kernel is touched)
ECDSA_DEPS := $(CSRC)/ecdsa_verify.h $(CSRC)/fe_secp256k1.h $(CSRC)/sc_secp256k1.h $(CSRC)/ge_secp256k1.h $(CSRC)/safegcd30.h $(CSRC)/sha256.h
$(CSRC)/ecdsa_verify.o: $(CSRC)/ecdsa_verify.hip $(ECDSA_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# ECDSA P-256 verification: its own lane code and object (the secp256k1 kernels are not touched)
ECDSA_P256_DEPS := $(CSRC)/ecdsa_p256_verify.h $(CSRC)/fe_p256.h $(CSRC)/sc_p256.h $(CSRC)/ge_p256.h $(ECDSA_DEPS)
$(CSRC)/ecdsa_p256_verify.o: $(CSRC)/ecdsa_p256_verify.hip $(ECDSA_P256_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/cbft_ecdsa.o: $(CSRC)/cbft_ecdsa.cpp $(INTERNAL_DEPS) $(ECDSA_P256_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# ECDSA secp256k1 signing: its own objects (constant-time lane code; ecdsa_verify.hip is not touched)
ECDSA_SIGN_DEPS := $(CSRC)/ecdsa_sign.h $(ECDSA_DEPS)
$(CSRC)/ecdsa_sign.o: $(CSRC)/ecdsa_sign.hip $(ECDSA_SIGN_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# ECDSA P-256 signing: its own lane code and object (constant-time; no other kernel is touched)
ECDSA_P256_SIGN_DEPS := $(CSRC)/ecdsa_p256_sign.h $(CSRC)/ecdsa_sign.h $(ECDSA_P256_DEPS)
$(CSRC)/ecdsa_p256_sign.o: $(CSRC)/ecdsa_p256_sign.hip $(ECDSA_P256_SIGN_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/cbft_ecdsa_sign.o: $(CSRC)/cbft_ecdsa_sign.cpp $(INTERNAL_DEPS) $(ECDSA_SIGN_DEPS) $(ECDSA_P256_SIGN_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/cbft_bls.o: $(CSRC)/cbft_bls.cpp $(INTERNAL_DEPS) $(CSRC)/bls_kernels.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB): $(CSRC)/ed25519_verify.o $(CSRC)/cbft_hipcrypto.o $(CSRC)/bls_kernels.o $(CSRC)/bls_msm_row.o $(CSRC)/bls_pairing.o $(CSRC)/bls_keys.o $(CSRC)/cbft_bls.o $(CSRC)/rsa_verify.o $(CSRC)/cbft_rsa.o $(CSRC)/ed25519_sign.o $(CSRC)/cbft_ed25519_sign.o $(CSRC)/rsa_sign.o $(CSRC)/cbft_rsa_sign.o $(CSRC)/bls_sign_batch.o $(CSRC)/cbft_bls_sign.o $(CSRC)/bls_verify_batch.o $(CSRC)/cbft_bls_verify_batch.o $(CSRC)/bls_combine_batch.o $(CSRC)/cbft_bls_combine_batch.o $(CSRC)/bls_multisig_batch.o $(CSRC)/cbft_bls_multisig_batch.o $(CSRC)/bls_keygen_batch.o $(CSRC)/cbft_bls_keygen.o $(CSRC)/ecdsa_verify.o $(CSRC)/cbft_ecdsa.o $(CSRC)/ecdsa_sign.o $(CSRC)/cbft_ecdsa_sign.o $(CSRC)/ecdsa_p256_verify.o $(CSRC)/ecdsa_p256_sign.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

oracle: $(ORACLE_LIB)

$(ORACLE_LIB): oracle/ed25519_oracle.c oracle/sha512_oracle.h
	gcc -O2 -std=c11 -fPIC -shared -Wall -o $@ oracle/ed25519_oracle.c

clean:
	rm -f $(CSRC)/*.o $(LIB) $(ORACLE_LIB)

CPU_LIB := tools/cpu_baseline/libcbft_cpu_openssl.so
cpu: $(CPU_LIB)
$(CPU_LIB): tools/cpu_baseline/openssl_ed25519.c
	gcc -O2 -std=gnu11 -fPIC -shared -Wall -Wno-deprecated-declarations -o $@ $< -lcrypto -lpthread
# the ECDSA secp256k1 host baseline of tools/ecdsa_bench.py (threads of ECDSA_do_verify)
CPU_ECDSA_LIB := tools/cpu_baseline/libcbft_cpu_openssl_ecdsa.so
cpu: $(CPU_ECDSA_LIB)
$(CPU_ECDSA_LIB): tools/cpu_baseline/openssl_ecdsa.c
	gcc -O2 -std=gnu11 -fPIC -shared -Wall -Wno-deprecated-declarations -o $@ $< -lcrypto -lpthread

# the ECDSA P-256 host baseline of tools/ecdsa_p256_bench.py (threads of ECDSA_do_verify on prime256v1)
CPU_P256_LIB := tools/cpu_baseline/libcbft_cpu_openssl_ecdsa_p256.so
cpu: $(CPU_P256_LIB)
$(CPU_P256_LIB): tools/cpu_baseline/openssl_ecdsa_p256.c
	gcc -O2 -std=gnu11 -fPIC -shared -Wall -Wno-deprecated-declarations -o $@ $< -lcrypto -lpthread

# the ECDSA secp256k1 signing host baseline of tools/ecdsa_sign_bench.py (threads of ECDSA_do_sign)
CPU_ECDSA_SIGN_LIB := tools/cpu_baseline/libcbft_cpu_openssl_ecdsa_sign.so
cpu: $(CPU_ECDSA_SIGN_LIB)
$(CPU_ECDSA_SIGN_LIB): tools/cpu_baseline/openssl_ecdsa_sign.c
	gcc -O2 -std=gnu11 -fPIC -shared -Wall -Wno-deprecated-declarations -o $@ $< -lcrypto -lpthread

# the ECDSA P-256 signing host baseline of tools/ecdsa_p256_sign_bench.py (threads of ECDSA_do_sign on prime256v1)
CPU_P256_SIGN_LIB := tools/cpu_baseline/libcbft_cpu_openssl_ecdsa_p256_sign.so
cpu: $(CPU_P256_SIGN_LIB)
$(CPU_P256_SIGN_LIB): tools/cpu_baseline/openssl_ecdsa_p256_sign.c
	gcc -O2 -std=gnu11 -fPIC -shared -Wall -Wno-deprecated-declarations -o $@ $< -lcrypto -lpthread

# C++ plugin layer.  Product sources (concord::hip, BLS::Hip) compile against the reference's own
# headers in an integration build (tests/test_reference_boundary.py) and here against the
# restatements in ref_mirror/ (the reference's util / bftengine / threshsign libraries need
# Crypto++, RELIC and CMF-generated code that the image does not have).
HOST_LIB := concord-bft_amd/libcbft_host.so
HOST_DIR := concord-bft_amd/host
HOST_SRC := $(HOST_DIR)/src/hip_ed25519.cpp $(HOST_DIR)/src/hip_rsa.cpp $(HOST_DIR)/src/hip_ecdsa.cpp $(HOST_DIR)/src/bls_hip.cpp $(HOST_DIR)/src/request_batch.cpp
MIRROR_SRC := $(wildcard $(HOST_DIR)/ref_mirror/src/*.cpp)
HOST_INC := -Iinclude -I$(HOST_DIR)/include -I$(HOST_DIR)/ref_mirror/include -DCBFT_WITH_CLIENT_KEYS_MAP
HOST_HDRS := $(wildcard $(HOST_DIR)/include/*.hpp $(HOST_DIR)/include/threshsign/*.hpp $(HOST_DIR)/ref_mirror/include/*.hpp $(HOST_DIR)/ref_mirror/include/threshsign/*.h)
host: $(HOST_LIB) tests/cpp/test_host tests/cpp/test_bls_host tests/cpp/test_sign_host tests/cpp/test_rsa_sign_host tests/cpp/test_bls_sign_host tests/cpp/test_bls_verify_host tests/cpp/test_bls_combine_host tests/cpp/test_bls_combine_plan_san tests/cpp/test_bls_multisig_host tests/cpp/test_bls_multisig_plan_san tests/cpp/test_bls_keygen_host tests/cpp/test_bls_keygen_san tests/cpp/test_ecdsa_host tests/cpp/test_ecdsa_sign_host tests/cpp/test_ecdsa_p256_host tests/cpp/test_ecdsa_p256_host_san tests/cpp/test_ecdsa_p256_sign_host tests/cpp/test_ecdsa_p256_sign_host_san tools/host_bench
$(HOST_LIB): $(HOST_SRC) $(MIRROR_SRC) $(HOST_HDRS) $(LIB) $(ECDSA_SIGN_DEPS) $(ECDSA_P256_SIGN_DEPS) $(CSRC)/ecdsa_der.h
	g++ -O2 -std=c++17 -fPIC -shared -Wall -Wno-unknown-pragmas $(HOST_INC) -o $@ $(HOST_SRC) $(MIRROR_SRC) -Lconcord-bft_amd -lcbft_hipcrypto -lcrypto -Wl,-rpath,'$$ORIGIN'
tests/cpp/test_host: tests/cpp/test_host.cpp $(HOST_LIB)
	g++ -O2 -std=c++17 -Wall -DCONCORD_BFT_TESTING $(HOST_INC) -o $@ $< -Lconcord-bft_amd -lcbft_host -lcbft_hipcrypto -lcrypto -lpthread -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

tests/cpp/test_sign_host: tests/cpp/test_sign_host.cpp $(HOST_LIB)
	g++ -O2 -std=c++17 -Wall $(HOST_INC) -o $@ $< -Lconcord-bft_amd -lcbft_host -lcbft_hipcrypto -lcrypto -lpthread -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

tests/cpp/test_rsa_sign_host: tests/cpp/test_rsa_sign_host.cpp $(HOST_LIB)
	g++ -O2 -std=c++17 -Wall $(HOST_INC) -o $@ $< -Lconcord-bft_amd -lcbft_host -lcbft_hipcrypto -lcrypto -lpthread -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

tests/cpp/test_bls_sign_host: tests/cpp/test_bls_sign_host.cpp $(HOST_LIB)
	g++ -O2 -std=c++17 -Wall $(HOST_INC) -o $@ $< -Lconcord-bft_amd -lcbft_host -lcbft_hipcrypto -lcrypto -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

tests/cpp/test_bls_verify_host: tests/cpp/test_bls_verify_host.cpp $(HOST_LIB)
	g++ -O2 -std=c++17 -Wall $(HOST_INC) -o $@ $< -Lconcord-bft_amd -lcbft_host -lcbft_hipcrypto -lcrypto -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

tests/cpp/test_bls_combine_host: tests/cpp/test_bls_combine_host.cpp $(HOST_LIB)
	g++ -O2 -std=c++17 -Wall $(HOST_INC) -o $@ $< -Lconcord-bft_amd -lcbft_host -lcbft_hipcrypto -lcrypto -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

# the same test with the host sources compiled in under ASan + UBSan, for its --no-gpu mode (the planning of
# combineBatch; run by tests/test_cpp_bls_combine_host.py as a stand-alone program, never loaded into python)
tests/cpp/test_bls_combine_plan_san: tests/cpp/test_bls_combine_host.cpp $(HOST_SRC) $(MIRROR_SRC) $(HOST_HDRS) $(LIB)
	g++ -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -Wno-unknown-pragmas $(HOST_INC) -o $@ $< $(HOST_SRC) $(MIRROR_SRC) -Lconcord-bft_amd -lcbft_hipcrypto -lcrypto -lpthread -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

tests/cpp/test_bls_multisig_host: tests/cpp/test_bls_multisig_host.cpp $(HOST_LIB)
	g++ -O2 -std=c++17 -Wall $(HOST_INC) -o $@ $< -Lconcord-bft_amd -lcbft_host -lcbft_hipcrypto -lcrypto -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

# the same test with the host sources compiled in under ASan + UBSan, for its --no-gpu mode (the planning of the
# multisig verifyBatch; run by tests/test_cpp_bls_multisig_host.py as a stand-alone program, never loaded into python)
tests/cpp/test_bls_multisig_plan_san: tests/cpp/test_bls_multisig_host.cpp $(HOST_SRC) $(MIRROR_SRC) $(HOST_HDRS) $(LIB)
	g++ -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -Wno-unknown-pragmas $(HOST_INC) -o $@ $< $(HOST_SRC) $(MIRROR_SRC) -Lconcord-bft_amd -lcbft_hipcrypto -lcrypto -lpthread -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

tests/cpp/test_bls_keygen_host: tests/cpp/test_bls_keygen_host.cpp $(HOST_LIB)
	g++ -O2 -std=c++17 -Wall $(HOST_INC) -o $@ $< -Lconcord-bft_amd -lcbft_host -lcbft_hipcrypto -lcrypto -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

# the same test with the host sources compiled in under ASan + UBSan, for its --no-gpu mode (sampling bounds, key
# encodings, the crossover setting; run by tests/test_cpp_bls_keygen_host.py as a stand-alone program, never loaded into python)
tests/cpp/test_bls_keygen_san: tests/cpp/test_bls_keygen_host.cpp $(HOST_SRC) $(MIRROR_SRC) $(HOST_HDRS) $(LIB)
	g++ -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -Wno-unknown-pragmas $(HOST_INC) -o $@ $< $(HOST_SRC) $(MIRROR_SRC) -Lconcord-bft_amd -lcbft_hipcrypto -lcrypto -lpthread -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

tests/cpp/test_ecdsa_host: tests/cpp/test_ecdsa_host.cpp $(HOST_LIB)
	g++ -O2 -std=c++17 -Wall -Wno-deprecated-declarations $(HOST_INC) -o $@ $< -Lconcord-bft_amd -lcbft_host -lcbft_hipcrypto -lcrypto -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

tests/cpp/test_ecdsa_p256_host: tests/cpp/test_ecdsa_p256_host.cpp $(HOST_LIB)
	g++ -O2 -std=c++17 -Wall -Wno-deprecated-declarations $(HOST_INC) -o $@ $< -Lconcord-bft_amd -lcbft_host -lcbft_hipcrypto -lcrypto -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

# the same test with the host sources compiled in under ASan + UBSan, for its --no-gpu mode (key parsing, the DER
# front end, the host path; run by tests/test_cpp_ecdsa_p256_host.py as a stand-alone program, never loaded into python)
tests/cpp/test_ecdsa_p256_host_san: tests/cpp/test_ecdsa_p256_host.cpp $(HOST_SRC) $(MIRROR_SRC) $(HOST_HDRS) $(LIB) $(CSRC)/ecdsa_der.h
	g++ -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -Wno-unknown-pragmas -Wno-deprecated-declarations $(HOST_INC) -o $@ $< $(HOST_SRC) $(MIRROR_SRC) -Lconcord-bft_amd -lcbft_hipcrypto -lcrypto -lpthread -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

tests/cpp/test_ecdsa_p256_sign_host: tests/cpp/test_ecdsa_p256_sign_host.cpp $(HOST_LIB)
	g++ -O2 -std=c++17 -Wall -Wno-deprecated-declarations $(HOST_INC) -o $@ $< -Lconcord-bft_amd -lcbft_host -lcbft_hipcrypto -lcrypto -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

# the same test with the host sources compiled in under ASan + UBSan, for its --no-gpu mode (key parsing, the lane code
# on the host, the DER writer; run by tests/test_cpp_ecdsa_p256_sign_host.py as a stand-alone program, never loaded into python)
tests/cpp/test_ecdsa_p256_sign_host_san: tests/cpp/test_ecdsa_p256_sign_host.cpp $(HOST_SRC) $(MIRROR_SRC) $(HOST_HDRS) $(LIB) $(ECDSA_P256_SIGN_DEPS) $(CSRC)/ecdsa_der.h
	g++ -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -Wno-unknown-pragmas -Wno-deprecated-declarations $(HOST_INC) -o $@ $< $(HOST_SRC) $(MIRROR_SRC) -Lconcord-bft_amd -lcbft_hipcrypto -lcrypto -lpthread -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

tests/cpp/test_ecdsa_sign_host: tests/cpp/test_ecdsa_sign_host.cpp $(HOST_LIB)
	g++ -O2 -std=c++17 -Wall -Wno-deprecated-declarations $(HOST_INC) -o $@ $< -Lconcord-bft_amd -lcbft_host -lcbft_hipcrypto -lcrypto -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

tests/cpp/test_bls_host: tests/cpp/test_bls_host.cpp $(HOST_LIB)
	g++ -O2 -std=c++17 -Wall $(HOST_INC) -o $@ $< -Lconcord-bft_amd -lcbft_host -lcbft_hipcrypto -lcrypto -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'

# per-request path benchmark (bench.py --full runs it): threads calling verify() / verifySig()
tools/host_bench: tools/host_bench.cpp $(HOST_LIB)
	g++ -O2 -std=c++17 -Wall -DCONCORD_BFT_TESTING $(HOST_INC) -o $@ $< -Lconcord-bft_amd -lcbft_host -lcbft_hipcrypto -lcrypto -lpthread -Wl,-rpath,'$$ORIGIN/../concord-bft_amd'

# host build of the BN-P254 device code, for the CPU tests (and the "not RELIC" CPU baseline)
SHIM := tests/cpp/libbn254_shim.so
shim: $(SHIM)
$(SHIM): tests/cpp/bn254_shim.cpp $(CSRC)/bn254_*.h $(CSRC)/bls_ops.h $(CSRC)/sha256.h
	g++ -O3 -funroll-loops -std=c++17 -fPIC -shared -Wall -Wno-unknown-pragmas -I$(CSRC) -o $@ $< -lpthread

# host build of the batched BLS signing lane routine (bls_sign_batch.h) for tests/test_bls_sign_cpu.py
BLS_SIGN_SHIM := tests/cpp/libbls_sign_shim.so
bls_sign_shim: $(BLS_SIGN_SHIM)
$(BLS_SIGN_SHIM): tests/cpp/bls_sign_shim.cpp $(CSRC)/bls_sign_batch.h $(CSRC)/bn254_*.h $(CSRC)/bls_ops.h $(CSRC)/sha256.h
	g++ -O3 -funroll-loops -std=c++17 -fPIC -shared -Wall -Wno-unknown-pragmas -I$(CSRC) -o $@ $< -lpthread

# host build of the batched BLS combination lane code (bls_combine_batch.h) for tests/test_bls_combine_batch_cpu.py,
# and the same source as a stand-alone program under ASan + UBSan (run by that test, never loaded into python)
BLS_COMBINE_SHIM := tests/cpp/libbls_combine_shim.so
BLS_COMBINE_SHIM_SAN := tests/cpp/bls_combine_shim_san
BLS_COMBINE_SHIM_DEPS := tests/cpp/bls_combine_shim.cpp $(CSRC)/bls_combine_batch.h $(CSRC)/bls_sign_batch.h $(CSRC)/bn254_*.h $(CSRC)/bls_ops.h $(CSRC)/sha256.h
bls_combine_shim: $(BLS_COMBINE_SHIM) $(BLS_COMBINE_SHIM_SAN)
$(BLS_COMBINE_SHIM): $(BLS_COMBINE_SHIM_DEPS)
	g++ -O3 -funroll-loops -std=c++17 -fPIC -shared -Wall -Wno-unknown-pragmas -I$(CSRC) -o $@ $<
$(BLS_COMBINE_SHIM_SAN): $(BLS_COMBINE_SHIM_DEPS)
	g++ -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -Wno-unknown-pragmas -DBLS_COMBINE_SHIM_MAIN -I$(CSRC) -o $@ $<

# host build of the batched BLS key derivation and dealing lane code (bls_keygen_batch.h) for tests/test_bls_keygen_cpu.py,
# and the same source as a stand-alone program under ASan + UBSan (run by that test, never loaded into python)
BLS_KEYGEN_SHIM := tests/cpp/libbls_keygen_shim.so
BLS_KEYGEN_SHIM_SAN := tests/cpp/bls_keygen_shim_san
BLS_KEYGEN_SHIM_DEPS := tests/cpp/bls_keygen_shim.cpp $(CSRC)/bls_keygen_batch.h $(CSRC)/bls_sign_batch.h $(CSRC)/bn254_*.h $(CSRC)/bls_ops.h $(CSRC)/sha256.h
bls_keygen_shim: $(BLS_KEYGEN_SHIM) $(BLS_KEYGEN_SHIM_SAN)
$(BLS_KEYGEN_SHIM): $(BLS_KEYGEN_SHIM_DEPS)
	g++ -O3 -funroll-loops -std=c++17 -fPIC -shared -Wall -Wno-unknown-pragmas -I$(CSRC) -o $@ $< -lpthread
$(BLS_KEYGEN_SHIM_SAN): $(BLS_KEYGEN_SHIM_DEPS)
	g++ -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -Wno-unknown-pragmas -DBLS_KEYGEN_SHIM_MAIN -I$(CSRC) -o $@ $< -lpthread

# host build of the row-parallel GF(2^255 - 19) code (fe25519_row.h) for tests/test_fe_row.py
FE_ROW_SHIM := tests/cpp/libfe_row_shim.so
fe_row_shim: $(FE_ROW_SHIM)
$(FE_ROW_SHIM): tests/cpp/fe_row_shim.cpp tests/cpp/row_emu.h $(CSRC)/fe25519_row.h $(CSRC)/row_lanes.h
	g++ -O2 -std=c++17 -fPIC -shared -Wall -Wno-unknown-pragmas -I$(CSRC) -Itests/cpp -o $@ $<

# host build of the fixed-length SHA-512 front end (sha512.h) for tests/test_sha512_fixed_cpu.py, and
# the same source as a stand-alone program under ASan + UBSan (run by that test, never loaded into python)
SHA512_SHIM := tests/cpp/libsha512_shim.so
SHA512_SHIM_SAN := tests/cpp/sha512_shim_san
sha512_shim: $(SHA512_SHIM) $(SHA512_SHIM_SAN)
$(SHA512_SHIM): tests/cpp/sha512_shim.cpp $(CSRC)/sha512.h
	g++ -O2 -std=c++17 -fPIC -shared -Wall -Wno-unknown-pragmas -I$(CSRC) -o $@ $<
$(SHA512_SHIM_SAN): tests/cpp/sha512_shim.cpp $(CSRC)/sha512.h
	g++ -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -Wno-unknown-pragmas -DSHA512_SHIM_MAIN -I$(CSRC) -o $@ $<

# host build of the ECDSA secp256k1 lane code (ecdsa_verify.h) for tests/test_ecdsa_cpu.py, and the
# same source as a stand-alone program under ASan + UBSan (run by that test, never loaded into python)
ECDSA_SHIM := tests/cpp/libecdsa_shim.so
ECDSA_SHIM_SAN := tests/cpp/ecdsa_shim_san
ecdsa_shim: $(ECDSA_SHIM) $(ECDSA_SHIM_SAN)
$(ECDSA_SHIM): tests/cpp/ecdsa_shim.cpp $(ECDSA_DEPS)
	g++ -O2 -std=c++17 -fPIC -shared -Wall -Wno-unknown-pragmas -I$(CSRC) -o $@ $<
$(ECDSA_SHIM_SAN): tests/cpp/ecdsa_shim.cpp $(ECDSA_DEPS)
	g++ -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -Wno-unknown-pragmas -DECDSA_SHIM_MAIN -I$(CSRC) -o $@ $<

# host build of the ECDSA secp256k1 signing lane code (ecdsa_sign.h) for tests/test_ecdsa_sign_cpu.py, and
# the same source as a stand-alone program under ASan + UBSan (run by that test, never loaded into python)
ECDSA_SIGN_SHIM := tests/cpp/libecdsa_sign_shim.so
ECDSA_SIGN_SHIM_SAN := tests/cpp/ecdsa_sign_shim_san
ecdsa_sign_shim: $(ECDSA_SIGN_SHIM) $(ECDSA_SIGN_SHIM_SAN)
$(ECDSA_SIGN_SHIM): tests/cpp/ecdsa_sign_shim.cpp $(ECDSA_SIGN_DEPS)
	g++ -O2 -std=c++17 -fPIC -shared -Wall -Wno-unknown-pragmas -I$(CSRC) -o $@ $< -lpthread
$(ECDSA_SIGN_SHIM_SAN): tests/cpp/ecdsa_sign_shim.cpp $(ECDSA_SIGN_DEPS)
	g++ -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -Wno-unknown-pragmas -DECDSA_SIGN_SHIM_MAIN -I$(CSRC) -o $@ $< -lpthread

# host build of the ECDSA P-256 lane code (ecdsa_p256_verify.h) and the DER front end (ecdsa_der.h) for
# tests/test_ecdsa_p256_cpu.py and tests/test_ecdsa_der_cpu.py, and the same source as a stand-alone program
# under ASan + UBSan (run by the former, never loaded into python)
ECDSA_P256_SHIM := tests/cpp/libecdsa_p256_shim.so
ECDSA_P256_SHIM_SAN := tests/cpp/ecdsa_p256_shim_san
ecdsa_p256_shim: $(ECDSA_P256_SHIM) $(ECDSA_P256_SHIM_SAN)
$(ECDSA_P256_SHIM): tests/cpp/ecdsa_p256_shim.cpp $(ECDSA_P256_DEPS) $(CSRC)/ecdsa_der.h
	g++ -O2 -std=c++17 -fPIC -shared -Wall -Wno-unknown-pragmas -I$(CSRC) -o $@ $<
$(ECDSA_P256_SHIM_SAN): tests/cpp/ecdsa_p256_shim.cpp $(ECDSA_P256_DEPS) $(CSRC)/ecdsa_der.h
	g++ -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -Wno-unknown-pragmas -DECDSA_P256_SHIM_MAIN -I$(CSRC) -o $@ $<

# host build of the ECDSA P-256 signing lane code (ecdsa_p256_sign.h) and the DER writer (ecdsa_der.h) for
# tests/test_ecdsa_p256_sign_cpu.py, and the same source as a stand-alone program under ASan + UBSan (run by that
# test, never loaded into python)
ECDSA_P256_SIGN_SHIM := tests/cpp/libecdsa_p256_sign_shim.so
ECDSA_P256_SIGN_SHIM_SAN := tests/cpp/ecdsa_p256_sign_shim_san
ecdsa_p256_sign_shim: $(ECDSA_P256_SIGN_SHIM) $(ECDSA_P256_SIGN_SHIM_SAN)
$(ECDSA_P256_SIGN_SHIM): tests/cpp/ecdsa_p256_sign_shim.cpp $(ECDSA_P256_SIGN_DEPS) $(CSRC)/ecdsa_der.h
	g++ -O2 -std=c++17 -fPIC -shared -Wall -Wno-unknown-pragmas -I$(CSRC) -o $@ $< -lpthread
$(ECDSA_P256_SIGN_SHIM_SAN): tests/cpp/ecdsa_p256_sign_shim.cpp $(ECDSA_P256_SIGN_DEPS) $(CSRC)/ecdsa_der.h
	g++ -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -Wno-unknown-pragmas -DECDSA_P256_SIGN_SHIM_MAIN -I$(CSRC) -o $@ $< -lpthread

# the front ends' HIP-free helpers (cbft_host_util.h) as a stand-alone program under ASan + UBSan
# (run by tests/test_host_util_cpu.py, never loaded into python)
HOST_UTIL_TEST := tests/cpp/host_util_test
host_util_test: $(HOST_UTIL_TEST)
$(HOST_UTIL_TEST): tests/cpp/host_util_test.cpp $(CSRC)/cbft_host_util.h
	g++ -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -I$(CSRC) -o $@ $<

# Host-layer sanitizer builds (host code only: the HIP library itself is not instrumented).
# ASan+UBSan and TSan variants of the C++ host library and its tests; run on a GPU box with
# tools/sanitize.sh.
SAN_DIR := tests/cpp/san
sanitize: $(LIB) $(MIRROR_SRC) $(HOST_SRC)
	mkdir -p $(SAN_DIR)
	for s in address,undefined thread; do \
	  t=$$(echo $$s | cut -d, -f1); \
	  g++ -O1 -g -fno-omit-frame-pointer -fsanitize=$$s -std=c++17 -fPIC -shared $(HOST_INC) -o $(SAN_DIR)/libcbft_host_$$t.so $(HOST_SRC) $(MIRROR_SRC) -Lconcord-bft_amd -lcbft_hipcrypto -lcrypto -lpthread -Wl,-rpath,'$$ORIGIN/../../../concord-bft_amd' && \
	  g++ -O1 -g -fno-omit-frame-pointer -fsanitize=$$s -std=c++17 -DCONCORD_BFT_TESTING $(HOST_INC) -o $(SAN_DIR)/test_host_$$t tests/cpp/test_host.cpp -L$(SAN_DIR) -lcbft_host_$$t -Lconcord-bft_amd -lcbft_hipcrypto -lcrypto -lpthread -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,'$$ORIGIN/../../../concord-bft_amd' && \
	  g++ -O1 -g -fno-omit-frame-pointer -fsanitize=$$s -std=c++17 $(HOST_INC) -o $(SAN_DIR)/test_sign_host_$$t tests/cpp/test_sign_host.cpp -L$(SAN_DIR) -lcbft_host_$$t -Lconcord-bft_amd -lcbft_hipcrypto -lcrypto -lpthread -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,'$$ORIGIN/../../../concord-bft_amd' && \
	  g++ -O1 -g -fno-omit-frame-pointer -fsanitize=$$s -std=c++17 $(HOST_INC) -o $(SAN_DIR)/test_bls_sign_host_$$t tests/cpp/test_bls_sign_host.cpp -L$(SAN_DIR) -lcbft_host_$$t -Lconcord-bft_amd -lcbft_hipcrypto -lcrypto -lpthread -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,'$$ORIGIN/../../../concord-bft_amd' && \
	  g++ -O1 -g -fno-omit-frame-pointer -fsanitize=$$s -std=c++17 $(HOST_INC) -o $(SAN_DIR)/test_bls_verify_host_$$t tests/cpp/test_bls_verify_host.cpp -L$(SAN_DIR) -lcbft_host_$$t -Lconcord-bft_amd -lcbft_hipcrypto -lcrypto -lpthread -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,'$$ORIGIN/../../../concord-bft_amd' && \
	  g++ -O1 -g -fno-omit-frame-pointer -fsanitize=$$s -std=c++17 $(HOST_INC) -o $(SAN_DIR)/test_bls_host_$$t tests/cpp/test_bls_host.cpp -L$(SAN_DIR) -lcbft_host_$$t -Lconcord-bft_amd -lcbft_hipcrypto -lcrypto -lpthread -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,'$$ORIGIN/../../../concord-bft_amd' || exit 1; \
	done

# Microbenchmarks and probes under tools/microbench (not part of `all`; `make microbench`).
MB := tools/microbench
MICROBENCH := $(MB)/intrate $(MB)/intrate2 $(MB)/concurrency $(MB)/rowfp $(MB)/permlane_check $(MB)/pack_probe
microbench: $(MICROBENCH)
$(MB)/%: $(MB)/%.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -I$(CSRC) -Iinclude -o $@ $<
# ISA probe of the P-256 field product under both reductions: `make p256_isa` prints the
# per-kernel instruction counts
p256_isa: tools/isa/p256_fe_mul_probe.hip $(CSRC)/fe_p256.h
	$(HIPCC) -S --cuda-device-only --offload-arch=$(ARCH) -O3 -std=c++17 -I$(CSRC) $< -o tools/isa/p256_fe_mul_probe.s
	python3 tools/isa/p256_fe_mul_count.py tools/isa/p256_fe_mul_probe.s
.PHONY: p256_isa
$(MB)/pack_probe: $(MB)/pack_probe.cpp
	$(HIPCC) -O2 -std=c++17 -o $@ $< -lpthread
.PHONY: microbench

# test-only device harness of the wave inversion (tests/test_inv_gpu.py; not the product library)
SELFTEST := tests/hip/libinv_selftest.so
SIGN_SELFTEST := tests/hip/libsign_selftest.so
RSA_SIGN_SELFTEST := tests/hip/librsa_sign_selftest.so
BLS_SIGN_SELFTEST := tests/hip/libbls_sign_selftest.so
BLS_VERIFY_SELFTEST := tests/hip/libbls_verify_selftest.so
BLS_COMBINE_SELFTEST := tests/hip/libbls_combine_selftest.so
FE25519_SELFTEST := tests/hip/libfe25519_selftest.so
ECDSA_SIGN_SELFTEST := tests/hip/libecdsa_sign_selftest.so
BLS_KEYGEN_SELFTEST := tests/hip/libbls_keygen_selftest.so
ECDSA_P256_SELFTEST := tests/hip/libecdsa_p256_selftest.so
ECDSA_P256_SIGN_SELFTEST := tests/hip/libecdsa_p256_sign_selftest.so
selftest: $(ECDSA_P256_SIGN_SELFTEST)
# test-only device harness of the ECDSA P-256 signing lane code, one function per launch (tests/test_ecdsa_p256_sign_gpu.py)
$(ECDSA_P256_SIGN_SELFTEST): tests/hip/ecdsa_p256_sign_selftest.hip $(CSRC)/ecdsa_p256_sign.hip $(ECDSA_P256_SIGN_DEPS)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<
selftest: $(SELFTEST) $(SIGN_SELFTEST) $(RSA_SIGN_SELFTEST) $(BLS_SIGN_SELFTEST) $(BLS_VERIFY_SELFTEST) $(BLS_COMBINE_SELFTEST) $(FE25519_SELFTEST) $(ECDSA_SIGN_SELFTEST) $(BLS_KEYGEN_SELFTEST) $(ECDSA_P256_SELFTEST)
# test-only device harness of the ECDSA P-256 field, scalar and point lane code, one function per launch
# (tests/test_ecdsa_p256_lane_gpu.py)
$(ECDSA_P256_SELFTEST): tests/hip/ecdsa_p256_selftest.hip $(ECDSA_P256_DEPS)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<
# test-only device harness of the ECDSA signing lane code, one function per launch (tests/test_ecdsa_sign_gpu.py)
$(ECDSA_SIGN_SELFTEST): tests/hip/ecdsa_sign_selftest.hip $(CSRC)/ecdsa_sign.hip $(ECDSA_SIGN_DEPS)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<
# test-only device harness of the Ed25519 field, scalar and point lane code, one function per launch
# (tests/test_fe25519_lane_gpu.py); ed25519_verify.o's flags, so ge_frombytes_row is compiled as in the product
$(FE25519_SELFTEST): tests/hip/fe25519_selftest.hip $(CSRC)/fe25519*.h $(CSRC)/ge25519.h $(CSRC)/sc25519.h $(CSRC)/safegcd30.h $(CSRC)/fe25519_row.h $(CSRC)/row_lanes.h
	$(HIPCC) $(HIPFLAGS) $(ROWFLAGS) -shared -o $@ $<
$(SELFTEST): tests/hip/inv_selftest.hip $(CSRC)/safegcd30.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<
# test-only device harness of the signing comb and sc_muladd (tests/test_ed25519_sign_gpu.py)
$(SIGN_SELFTEST): tests/hip/sign_selftest.hip $(CSRC)/ed25519_sign.h $(CSRC)/ge25519.h $(CSRC)/fe25519*.h $(CSRC)/sc25519.h $(CSRC)/sha512.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<
# test-only device harness of the RSA CRT core on raw EM integers (tests/test_rsa_sign_gpu.py)
$(RSA_SIGN_SELFTEST): tests/hip/rsa_sign_selftest.hip $(CSRC)/rsa_sign.h $(CSRC)/sha256.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<
# test-only device harness of the BLS signing lane code: the hash from a given x, and the product
# kernels beside their rejected variants (tests/test_bls_sign_gpu.py, tools/bls_sign_bench.py)
$(BLS_SIGN_SELFTEST): tests/hip/bls_sign_selftest.hip $(CSRC)/bls_sign_batch.h $(BLS_DEPS)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<
# test-only device harness of the batched BLS verification: the product kernels timed stage by stage
# (tools/bls_verify_bench.py)
$(BLS_VERIFY_SELFTEST): tests/hip/bls_verify_selftest.hip $(CSRC)/bls_verify_batch.hip $(CSRC)/bls_verify_batch.h $(CSRC)/bls_sign_batch.h $(BLS_DEPS) $(LIB)
	$(HIPCC) $(HIPFLAGS) $(ROWFLAGS) -shared -o $@ $< -Lconcord-bft_amd -lcbft_hipcrypto -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'
# test-only device harness of the batched BLS combination: the product kernels timed stage by stage, beside
# the constant-time signing kernel on the same points (tools/bls_combine_bench.py)
$(BLS_COMBINE_SELFTEST): tests/hip/bls_combine_selftest.hip $(CSRC)/bls_combine_batch.hip $(BLS_COMBINE_DEPS) $(LIB)
	$(HIPCC) $(HIPFLAGS) $(ROWFLAGS) -shared -o $@ $< -Lconcord-bft_amd -lcbft_hipcrypto -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'
# test-only device harness of the batched BLS key derivation: the product kernel beside the rejected geometry (the
# row-parallel comb over a grid), each timed (tools/bls_keygen_bench.py)
$(BLS_KEYGEN_SELFTEST): tests/hip/bls_keygen_selftest.hip $(CSRC)/bls_keygen_batch.hip $(BLS_KEYGEN_DEPS) $(LIB)
	$(HIPCC) $(HIPFLAGS) $(ROWFLAGS) -shared -o $@ $< -Lconcord-bft_amd -lcbft_hipcrypto -Wl,-rpath,'$$ORIGIN/../../concord-bft_amd'
