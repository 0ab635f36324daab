// abi_proof_common.inc — what the one-call provers share on the host beside their transcript script (proof_host.hpp) and their derived generator
// sets (abi_msm.inc: derived_set): a row commit whose points the host needs (rows_to_host_launch / _collect: the commit, the hand-over kernel, the
// one wait, affine bytes) and the envelope of a prover that keeps its transcript on the host (prove_on_copy).  The verifiers' counterpart is
// abi_verify_common.inc.  Included by sbn254.hip.

// `nrows` rows of R canonical scalars (and their blinds, or null) as ONE commit over `ext`; the XYZZ sums and the `nextra` words at `extra` that
// travel with them go to the host mailbox from word `slot_word` on, the flag to word `flag_word` — launches only; *seq is what
// rows_to_host_collect waits for.  A caller that keeps several commits in flight gives each its own words.
static int rows_to_host_launch(sbn_ctx* c, const sbn_bases* ext, const uint32_t* rows, const uint32_t* blinds, size_t nrows, size_t R, const uint32_t* extra, uint32_t nextra,
                               uint32_t slot_word, uint32_t flag_word, uint32_t* seq) {
  int rc;
  const uint32_t words = 32 * (uint32_t)nrows + nextra;
  if (nrows > (size_t)R1CS_SIGMA_ROWS_MAX || slot_word + words > (uint32_t)SC_MBOX_WORDS) return fail(c, SBN_EINVAL, "hand-over: %zu points and %u words from word %u on do not fit the host mailbox", nrows, nextra, slot_word);
  if ((rc = ensure(c, c->wsum, 4096))) return rc;                       // (the commit asks for nrows x 128 B; a caller with launches of its own ahead of this one sizes it before them)
  if ((rc = sc_tickets(c))) return rc;                                  // (for the host mailbox it allocates on first use; no ticket is taken)
  { RowInfo ri; ri.internal_rows = true;
    if ((rc = commit_rows_launch(c, ext, rows, blinds, nrows, R, nullptr, nullptr, ri))) return rc; }   // sums stay XYZZ in c->wsum: read by the next launch of the stream
  *seq = ++c->mbox_seq;
  LAUNCH(c, "k_points_to_host", k_points_to_host, 1, words <= 128 ? 128 : 256, (const uint32_t*)c->wsum.p, (uint32_t)nrows, extra, nextra, c->mbox + slot_word, c->mbox + flag_word, *seq);
  LAUNCHCHK(c);
  return SBN_OK;
}
// the one host wait of such a commit: the points as canonical affine bytes (npoints x 64; inf: npoints or null), the extra bytes that travelled with them.
// ONE inversion for all the points (a binary Euclid, 2-3 us on a host core)
static int rows_to_host_collect(sbn_ctx* c, uint32_t slot_word, uint32_t flag_word, uint32_t seq, size_t npoints, uint8_t* xy, int* inf, uint8_t* extra, size_t nextra_bytes) {
  int rc;
  if (npoints > (size_t)R1CS_SIGMA_ROWS_MAX) return fail(c, SBN_EINVAL, "hand-over: %zu points, at most %d are collected at once", npoints, R1CS_SIGMA_ROWS_MAX);
  if ((rc = sc_flag_wait(c, c->mbox + flag_word, seq))) return rc;
  const uint8_t* h = (const uint8_t*)(c->mbox + slot_word);
  sbn_host::Pt S[R1CS_SIGMA_ROWS_MAX]; memcpy(S, h, npoints * 128);
  for (size_t i = 0; i < npoints; i++) S[i] = sbn_host::pt_from_device(S[i]);
  if (npoints == 2) sbn_host::to_affine_bytes2(S[0], S[1], xy, inf, xy + 64, inf ? inf + 1 : nullptr);
  else sbn_host::to_affine_bytes_n(S, npoints, xy, inf);
  if (nextra_bytes) memcpy(extra, h + npoints * 128, nextra_bytes);
  return SBN_OK;
}

// The proof runs on a copy of the caller's transcript, which moves on only when `body` (an int(MerlinTranscript&)) returns SBN_OK.  Behind a
// failure nothing of the call stays queued: the stream is waited for, as TableScope does for the tables.  The caller holds the context's mutex.
template <class Body>
static int prove_on_copy(sbn_ctx* c, sbn_transcript* tr, Body body) {
  sbn_host::MerlinTranscript t = tr->t;
  const int rc = body(t);
  if (rc != SBN_OK) { hipStreamSynchronize(c->stream); return rc; }
  tr->t = t;
  return SBN_OK;
}
