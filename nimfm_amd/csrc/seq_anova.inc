// nimfm_amd/csrc/seq_anova.inc -- one order of predictWithGrad for thread tid's factor, as TEXT (seq_step.h says why): the ANOVA
// kernel of degree `deg` over the row (sgd.nim:152-170) and computeAnovaDerivative (sgd.nim:176-188) into dA[row.slot(o, q)].
// The including scope supplies the constants MAXDEG and SCALED, row, o, deg, m_tot, dA, sP (read when SCALED) and kv (the result).
{
  auto param = [&](int q) {
    if constexpr (SCALED) return sP * row.param(o, q);
    else return row.param(o, q);
  };
  double A[MAXDEG + 1];
  if (deg != 2) {  // sgd.nim:152-159
    A[0] = 1.0;
#pragma unroll
    for (int t = 1; t <= MAXDEG; ++t) A[t] = 0.0;
    for (int q = 0; q < m_tot; ++q) {
      const double val = row.value(q);
      const double p = param(q);
#pragma unroll
      for (int t = MAXDEG; t >= 1; --t)
        if (t <= deg) A[t] += A[t - 1] * p * val;
    }
#pragma unroll
    for (int t = 1; t <= MAXDEG; ++t)
      if (t == deg) kv = A[t];
  } else {  // sgd.nim:160-170
    double a1 = 0.0, a2 = 0.0;
    for (int q = 0; q < m_tot; ++q) {
      const double val = row.value(q);
      const double p = param(q);
      a1 += val * p;
      a2 += (val * p) * (val * p);
    }
    A[0] = 1.0;
    A[1] = a1;
    kv = (a1 * a1 - a2) / 2;
  }
  // computeAnovaDerivative: sgd.nim:176-188
  for (int q = 0; q < m_tot; ++q) {
    const double val = row.value(q);
    const double p = param(q);
    double d_;
    if (deg != 2) {
      d_ = val;
#pragma unroll
      for (int t = 1; t < MAXDEG; ++t)
        if (t < deg) d_ = val * (A[t] - p * d_);
    } else {
      d_ = val * (A[1] - p * val);
    }
    dA[row.slot(o, q)] = d_;
  }
}
