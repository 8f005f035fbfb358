/* transform.hip — the transform-function layer on the result grid
 * (SURVEY.md §8f(4), app/vmselect/promql/transform.go).
 *
 * Three device families over the [n_series x n_grid] result matrix:
 *   elementwise  one-arg math funcs (transform.go:26-131 one-arg table),
 *                clamp/clamp_min/clamp_max (:271-334), round (:2340),
 *                sgn (:2374), bitmap_and/or/xor (:2745), and the UTC
 *                date-time funcs (newTransformFuncDateTime :333 — Go
 *                time.Unix(int64(v),0).UTC() calendar math restated via
 *                the civil-from-days algorithm).
 *   per-series   sequential column walks: keep_last/next_value (:1232,
 *                :1255), interpolate (:1279), running_* (:1326),
 *                range_* (:1353-1680), smooth_exponential (:1682),
 *                remove_resets (:1731 removeCounterResetsMaybeNaNs
 *                :2929).  One thread per series; quantile-based funcs
 *                (range_quantile/trim_spikes/trim_outliers/mad) insertion-
 *                sort into a per-series global scratch column — transforms
 *                run on post-aggregation result sets (10^3-10^5 series),
 *                not the raw 10^6-series rollup input.
 *
 * Scalar args (clamp bounds, round nearest, bitmap masks, smoothing
 * factors) are per-grid-point rows exactly as the reference's getScalar
 * (eval args are series).  Label funcs (label_*, sort_*) are host metadata
 * work in victoriametrics_amd/transform.py.
 *
 * Go float->uint64 / float->int64 conversion semantics (bitmap funcs,
 * date funcs) follow Go-on-amd64: truncation toward zero; NaN and
 * out-of-range int64 -> INT64_MIN; uint64 via the 2^63-split Go emits.
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>

#include "host_common.h"
#include "../../include/vmgpu.h"

static __device__ __forceinline__ double t_nan() {
  return __longlong_as_double(0x7ff8000000000000LL);
}

/* Go int64(v) on amd64: cvttsd2si — truncate toward zero, NaN/overflow ->
 * INT64_MIN. */
static __device__ long long t_go_i64(double v) {
  if (isnan(v) || v >= 9.223372036854775808e18 || v < -9.223372036854775808e18)
    return (long long)0x8000000000000000LL;
  return (long long)v;
}

/* Go uint64(v) on amd64 (the 2^63 branchy lowering). */
static __device__ unsigned long long t_go_u64(double v) {
  if (v < 9.223372036854775808e18) return (unsigned long long)t_go_i64(v);
  return (unsigned long long)t_go_i64(v - 9.223372036854775808e18) +
         0x8000000000000000ULL;
}

/* ---- UTC calendar (civil-from-days; Go time.Unix(sec,0).UTC()) -------- */
struct TCivil { int y, m, d, yd; };

static __device__ TCivil t_civil_from_unix(long long sec, long long* rem) {
  long long days = sec / 86400;
  long long r = sec % 86400;
  if (r < 0) { r += 86400; days -= 1; }
  *rem = r;
  /* Howard Hinnant's civil_from_days */
  long long z = days + 719468;
  long long era = (z >= 0 ? z : z - 146096) / 146097;
  unsigned doe = (unsigned)(z - era * 146097);
  unsigned yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  long long y = (long long)yoe + era * 400;
  unsigned doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  unsigned mp = (5 * doy + 2) / 153;
  unsigned d = doy - (153 * mp + 2) / 5 + 1;
  unsigned m = mp < 10 ? mp + 3 : mp - 9;
  TCivil c;
  c.y = (int)(y + (m <= 2));
  c.m = (int)m;
  c.d = (int)d;
  /* day of year: days since Jan 1 of c.y, +1 */
  int leap = (c.y % 4 == 0 && (c.y % 100 != 0 || c.y % 400 == 0)) ? 1 : 0;
  static const int cum[13] = {0, 0, 31, 59, 90, 120, 151, 181, 212, 243,
                              273, 304, 334};
  c.yd = cum[c.m] + (c.m > 2 ? leap : 0) + c.d;
  return c;
}

static __device__ int t_days_in_month(int y, int m) {
  static const int dm[13] = {0, 31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
  int leap = (y % 4 == 0 && (y % 100 != 0 || y % 400 == 0)) ? 1 : 0;
  return (m == 2) ? 28 + leap : dm[m];
}

/* elementwise func body; a1/a2 are the per-point scalar-arg values */
static __device__ double t_elementwise(int f, double v, double a1, double a2) {
  switch (f) {
    case VMGPU_TF_ABS:   return fabs(v);
    case VMGPU_TF_CEIL:  return ceil(v);
    case VMGPU_TF_FLOOR: return floor(v);
    case VMGPU_TF_EXP:   return exp(v);
    case VMGPU_TF_LN:    return log(v);
    case VMGPU_TF_LOG2:  return log2(v);
    case VMGPU_TF_LOG10: return log10(v);
    case VMGPU_TF_SQRT:  return sqrt(v);
    case VMGPU_TF_SIN:   return sin(v);
    case VMGPU_TF_COS:   return cos(v);
    case VMGPU_TF_TAN:   return tan(v);
    case VMGPU_TF_ASIN:  return asin(v);
    case VMGPU_TF_ACOS:  return acos(v);
    case VMGPU_TF_ATAN:  return atan(v);
    case VMGPU_TF_SINH:  return sinh(v);
    case VMGPU_TF_COSH:  return cosh(v);
    case VMGPU_TF_TANH:  return tanh(v);
    case VMGPU_TF_ASINH: return asinh(v);
    case VMGPU_TF_ACOSH: return acosh(v);
    case VMGPU_TF_ATANH: return atanh(v);
    case VMGPU_TF_DEG:   return v * 180.0 / M_PI;
    case VMGPU_TF_RAD:   return v * M_PI / 180.0;
    case VMGPU_TF_SGN:   return (v < 0) ? -1.0 : (v > 0 ? 1.0 : 0.0);
    case VMGPU_TF_CLAMP:
      /* transformClamp (transform.go:271): min then max applied per point */
      if (v < a1) v = a1;
      if (v > a2) v = a2;
      return v;
    case VMGPU_TF_CLAMP_MIN: return (v < a1) ? a1 : v;
    case VMGPU_TF_CLAMP_MAX: return (v > a1) ? a1 : v;
    case VMGPU_TF_ROUND: {
      /* transformRound (transform.go:2340): a1 = nearest, a2 = p10
       * (10^-e of decimal.FromFloat(nearest), precomputed on the host —
       * the same nPrev caching the reference does, hoisted). */
      v += 0.5 * copysign(a1, v);
      v -= fmod(v, a1);
      double ipart;
      (void)modf(v * a2, &ipart);
      return ipart / a2;
    }
    case VMGPU_TF_BITMAP_AND:
      return (isnan(v) || isnan(a1)) ? t_nan()
             : (double)(t_go_u64(v) & t_go_u64(a1));
    case VMGPU_TF_BITMAP_OR:
      return (isnan(v) || isnan(a1)) ? t_nan()
             : (double)(t_go_u64(v) | t_go_u64(a1));
    case VMGPU_TF_BITMAP_XOR:
      return (isnan(v) || isnan(a1)) ? t_nan()
             : (double)(t_go_u64(v) ^ t_go_u64(a1));
    default: break;
  }
  /* date-time funcs: NaN passes through (newTransformFuncDateTime:347) */
  if (isnan(v)) return v;
  long long rem;
  TCivil c = t_civil_from_unix(t_go_i64(v), &rem);
  switch (f) {
    case VMGPU_TF_DAY_OF_MONTH:  return (double)c.d;
    case VMGPU_TF_DAY_OF_WEEK: {
      long long days = t_go_i64(v) / 86400;
      if (t_go_i64(v) % 86400 < 0) days -= 1;
      long long w = (days + 4) % 7;        /* 1970-01-01 was Thursday */
      if (w < 0) w += 7;
      return (double)w;                     /* Go Weekday: Sunday=0 */
    }
    case VMGPU_TF_DAY_OF_YEAR:   return (double)c.yd;
    case VMGPU_TF_DAYS_IN_MONTH: return (double)t_days_in_month(c.y, c.m);
    case VMGPU_TF_HOUR:          return (double)(rem / 3600);
    case VMGPU_TF_MINUTE:        return (double)((rem % 3600) / 60);
    case VMGPU_TF_MONTH:         return (double)c.m;
    case VMGPU_TF_YEAR:          return (double)c.y;
    default:                     return t_nan();
  }
}

__global__ void transform_elementwise_kernel(int func, double* values,
                                             uint64_t n_series, uint32_t n_grid,
                                             const double* arg1,
                                             const double* arg2) {
  uint64_t total = n_series * n_grid;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t g = (uint32_t)(e % n_grid);
    double a1 = arg1 ? arg1[g] : 0.0;
    double a2 = arg2 ? arg2[g] : 0.0;
    values[e] = t_elementwise(func, values[e], a1, a2);
  }
}

/* quantileSorted (aggr.go:922), bit-exact formulation */
static __device__ double t_quantile_sorted(double phi, const double* a, int n) {
  if (n == 0 || isnan(phi)) return t_nan();
  if (phi < 0) return __longlong_as_double(0xfff0000000000000LL);
  if (phi > 1) return __longlong_as_double(0x7ff0000000000000LL);
  double rank = phi * (double)(n - 1);
  double lower_idx = fmax(0.0, floor(rank));
  double upper_idx = fmin((double)(n - 1), lower_idx + 1.0);
  double weight = rank - floor(rank);
  return a[(int)lower_idx] * (1.0 - weight) + a[(int)upper_idx] * weight;
}

/* insertion-sort the non-NaN values of row into scratch; returns count */
static __device__ int t_sorted_nonnan(const double* row, uint32_t n,
                                      double* scratch) {
  int cnt = 0;
  for (uint32_t i = 0; i < n; i++) {
    double v = row[i];
    if (isnan(v)) continue;
    int j = cnt;
    while (j > 0 && scratch[j - 1] > v) {
      scratch[j] = scratch[j - 1];
      j--;
    }
    scratch[j] = v;
    cnt++;
  }
  return cnt;
}

static __device__ double t_mean(const double* row, uint32_t n) {
  double sum = 0.0;
  int cnt = 0;
  for (uint32_t i = 0; i < n; i++)
    if (!isnan(row[i])) { sum += row[i]; cnt++; }
  return sum / (double)cnt;   /* 0/0 = NaN, matching Go */
}

/* stdvar (rollup.go:1808 via stddevForValues) — Welford, matching the
 * reference's streaming formulation bit-for-bit */
static __device__ double t_stdvar(const double* row, uint32_t n) {
  double avg = 0.0, count = 0.0, q = 0.0;
  for (uint32_t i = 0; i < n; i++) {
    double v = row[i];
    if (isnan(v)) continue;
    count++;
    double avg_new = avg + (v - avg) / count;
    q += (v - avg) * (v - avg_new);
    avg = avg_new;
  }
  if (count == 0.0) return t_nan();
  return q / count;
}

__global__ void transform_series_kernel(int func, double* values,
                                        uint64_t n_series, uint32_t n_grid,
                                        const int64_t* ts,
                                        const double* arg1,  /* per-point row */
                                        double scalar_arg,
                                        double* scratch,     /* [n_series*n_grid] */
                                        uint8_t* keep_flags) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       s < n_series; s += (uint64_t)gridDim.x * blockDim.x) {
    double* row = values + s * n_grid;
    uint32_t n = n_grid;
    if (keep_flags) keep_flags[s] = 1;
    switch (func) {
      case VMGPU_TF_KEEP_LAST_VALUE: {  /* transform.go:1232 */
        if (n == 0) break;
        double last = row[0];
        for (uint32_t i = 0; i < n; i++) {
          if (!isnan(row[i])) last = row[i];
          else row[i] = last;
        }
        break;
      }
      case VMGPU_TF_KEEP_NEXT_VALUE: {  /* transform.go:1255 */
        if (n == 0) break;
        double next = row[n - 1];
        for (int i = (int)n - 1; i >= 0; i--) {
          if (!isnan(row[i])) next = row[i];
          else row[i] = next;
        }
        break;
      }
      case VMGPU_TF_INTERPOLATE: {      /* transform.go:1279 */
        uint32_t lo = 0, hi = n;
        while (lo < hi && isnan(row[lo])) lo++;
        while (hi > lo && isnan(row[hi - 1])) hi--;
        double prev = t_nan();
        for (uint32_t i = lo; i < hi; i++) {
          if (!isnan(row[i])) continue;
          if (i > lo) prev = row[i - 1];
          uint32_t j = i + 1;
          while (j < hi && isnan(row[j])) j++;
          double next = (j >= hi) ? prev : row[j];
          if (isnan(prev)) prev = next;
          double delta = (next - prev) / (double)(j - i + 1);
          while (i < j) {
            prev += delta;
            row[i] = prev;
            i++;
          }
        }
        break;
      }
      case VMGPU_TF_RUNNING_SUM:
      case VMGPU_TF_RUNNING_MIN:
      case VMGPU_TF_RUNNING_MAX:
      case VMGPU_TF_RUNNING_AVG:
      case VMGPU_TF_RANGE_SUM:
      case VMGPU_TF_RANGE_MIN:
      case VMGPU_TF_RANGE_MAX:
      case VMGPU_TF_RANGE_AVG: {        /* transform.go:1326,1353 */
        uint32_t lo = 0;
        while (lo < n && isnan(row[lo])) lo++;
        if (lo >= n) break;
        double prev = row[lo];
        for (uint32_t i = lo + 1; i < n; i++) {
          double v = row[i];
          int idx = (int)(i - lo);    /* rf idx starts at 1 */
          if (!isnan(v)) {
            switch (func) {
              case VMGPU_TF_RUNNING_SUM: case VMGPU_TF_RANGE_SUM:
                prev = prev + v; break;
              case VMGPU_TF_RUNNING_MIN: case VMGPU_TF_RANGE_MIN:
                prev = (prev < v) ? prev : v; break;
              case VMGPU_TF_RUNNING_MAX: case VMGPU_TF_RANGE_MAX:
                prev = (prev > v) ? prev : v; break;
              default:
                prev = prev + (v - prev) / (double)(idx + 1); break;
            }
          }
          row[i] = prev;
        }
        if (func >= VMGPU_TF_RANGE_SUM && func <= VMGPU_TF_RANGE_AVG) {
          /* setLastValues (transform.go:1670) */
          uint32_t hi = n;
          while (hi > 0 && isnan(row[hi - 1])) hi--;
          if (hi == 0) break;
          double last = row[hi - 1];
          for (uint32_t i = 0; i < n; i++) row[i] = last;
        }
        break;
      }
      case VMGPU_TF_RANGE_FIRST: {      /* transform.go:1638 */
        uint32_t lo = 0;
        while (lo < n && isnan(row[lo])) lo++;
        if (lo >= n) break;
        double first = row[lo];
        for (uint32_t i = 0; i < n; i++) row[i] = first;
        break;
      }
      case VMGPU_TF_RANGE_LAST: {       /* transform.go:1658 */
        uint32_t hi = n;
        while (hi > 0 && isnan(row[hi - 1])) hi--;
        if (hi == 0) break;
        double last = row[hi - 1];
        for (uint32_t i = 0; i < n; i++) row[i] = last;
        break;
      }
      case VMGPU_TF_RANGE_NORMALIZE: {  /* transform.go:1365 */
        double vmin = __longlong_as_double(0x7ff0000000000000LL);
        double vmax = -vmin;
        for (uint32_t i = 0; i < n; i++) {
          double v = row[i];
          if (isnan(v)) continue;
          if (v < vmin) vmin = v;
          if (v > vmax) vmax = v;
        }
        double d = vmax - vmin;
        if (isinf(d)) { if (keep_flags) keep_flags[s] = 0; break; }
        for (uint32_t i = 0; i < n; i++) row[i] = (row[i] - vmin) / d;
        break;
      }
      case VMGPU_TF_RANGE_ZSCORE:
      case VMGPU_TF_RANGE_TRIM_ZSCORE: {  /* transform.go:1397,1426 */
        double sd = sqrt(t_stdvar(row, n));
        double avg = t_mean(row, n);
        if (func == VMGPU_TF_RANGE_ZSCORE) {
          for (uint32_t i = 0; i < n; i++) row[i] = (row[i] - avg) / sd;
        } else {
          double z = fabs(scalar_arg);
          for (uint32_t i = 0; i < n; i++)
            if (fabs(row[i] - avg) / sd > z) row[i] = t_nan();
        }
        break;
      }
      case VMGPU_TF_RANGE_STDDEV:
      case VMGPU_TF_RANGE_STDVAR: {     /* transform.go:1568,1584 */
        double v = t_stdvar(row, n);
        if (func == VMGPU_TF_RANGE_STDDEV) v = sqrt(v);
        for (uint32_t i = 0; i < n; i++) row[i] = v;
        break;
      }
      case VMGPU_TF_RANGE_LINREG: {     /* transform.go:1531 */
        if (n == 0) break;
        /* linearRegression (rollup.go:1423): const fast path, NaN skip,
         * |tDiff| >= 1e-6 slope gate */
        int64_t t0 = ts[0];
        bool all_const = true;
        for (uint32_t i = 1; i < n && all_const; i++)
          all_const = (row[i] == row[0]);
        double v0, k;
        if (all_const) {
          v0 = row[0];
          k = 0.0;
        } else {
          double vsum = 0, tsum = 0, tvsum = 0, ttsum = 0, cnt = 0;
          for (uint32_t i = 0; i < n; i++) {
            double v = row[i];
            if (isnan(v)) continue;
            double dt = (double)(ts[i] - t0) / 1e3;
            cnt++;
            vsum += v;
            tsum += dt;
            tvsum += dt * v;
            ttsum += dt * dt;
          }
          if (cnt == 0) {
            v0 = t_nan();
            k = t_nan();
          } else {
            k = 0.0;
            double tdiff = ttsum - tsum * tsum / cnt;
            if (fabs(tdiff) >= 1e-6)
              k = (tvsum - tsum * vsum / cnt) / tdiff;
            v0 = vsum / cnt - k * tsum / cnt;
          }
        }
        for (uint32_t i = 0; i < n; i++)
          row[i] = v0 + k * (double)(ts[i] - t0) / 1e3;
        break;
      }
      case VMGPU_TF_RANGE_MAD:
      case VMGPU_TF_RANGE_TRIM_OUTLIERS: {  /* transform.go:1552,1455 */
        double* sc = scratch + s * n_grid;
        int cnt = t_sorted_nonnan(row, n, sc);
        double med = t_quantile_sorted(0.5, sc, cnt);
        /* mad (rollup.go:1476): median of |v - med| */
        /* quantile() drops NaN before it sorts: with an infinite median
         * the deviation of every sample equal to it is NaN and leaves */
        int dcnt = 0;
        for (int i = 0; i < cnt; i++) {
          double d = fabs(sc[i] - med);
          if (!isnan(d)) sc[dcnt++] = d;
        }
        /* re-sort the deviations */
        for (int i = 1; i < dcnt; i++) {
          double v = sc[i];
          int j = i;
          while (j > 0 && sc[j - 1] > v) { sc[j] = sc[j - 1]; j--; }
          sc[j] = v;
        }
        double madv = t_quantile_sorted(0.5, sc, dcnt);
        if (func == VMGPU_TF_RANGE_MAD) {
          for (uint32_t i = 0; i < n; i++) row[i] = madv;
        } else {
          double dmax = scalar_arg * madv;
          for (uint32_t i = 0; i < n; i++)
            if (fabs(row[i] - med) > dmax) row[i] = t_nan();
        }
        break;
      }
      case VMGPU_TF_RANGE_TRIM_SPIKES: {   /* transform.go:1483 */
        double* sc = scratch + s * n_grid;
        int cnt = t_sorted_nonnan(row, n, sc);
        double phi = scalar_arg / 2.0;
        double vmax = t_quantile_sorted(1.0 - phi, sc, cnt);
        double vmin = t_quantile_sorted(phi, sc, cnt);
        for (uint32_t i = 0; i < n; i++) {
          double v = row[i];
          if (isnan(v)) continue;
          if (v > vmax || v < vmin) row[i] = t_nan();
        }
        break;
      }
      case VMGPU_TF_RANGE_QUANTILE: {      /* transform.go:1600 */
        double* sc = scratch + s * n_grid;
        int last_idx = -1;
        int cnt = 0;
        for (uint32_t i = 0; i < n; i++) {
          double v = row[i];
          if (isnan(v)) continue;
          int j = cnt;
          while (j > 0 && sc[j - 1] > v) { sc[j] = sc[j - 1]; j--; }
          sc[j] = v;
          cnt++;
          last_idx = (int)i;
        }
        if (last_idx >= 0)
          row[last_idx] = t_quantile_sorted(scalar_arg, sc, cnt);
        /* setLastValues */
        uint32_t hi = n;
        while (hi > 0 && isnan(row[hi - 1])) hi--;
        if (hi == 0) break;
        double last = row[hi - 1];
        for (uint32_t i = 0; i < n; i++) row[i] = last;
        break;
      }
      case VMGPU_TF_SMOOTH_EXPONENTIAL: {  /* transform.go:1682 */
        uint32_t lo = 0;
        while (lo < n && isnan(row[lo])) lo++;
        while (lo < n && isinf(row[lo])) lo++;
        if (lo >= n) break;
        double avg = row[lo];
        for (uint32_t i = lo + 1; i < n; i++) {
          double v = row[i];
          if (isnan(v)) continue;
          if (isinf(v)) { row[i] = avg; continue; }
          double sf = arg1 ? arg1[i] : 1.0;
          if (isnan(sf)) sf = 1.0;
          if (sf < 0.0) sf = 0.0;
          if (sf > 1.0) sf = 1.0;
          avg = avg * (1.0 - sf) + v * sf;
          row[i] = avg;
        }
        break;
      }
      case VMGPU_TF_REMOVE_RESETS: {       /* transform.go:2929 */
        uint32_t lo = 0;
        while (lo < n && isnan(row[lo])) lo++;
        if (lo >= n) break;
        double corr = 0.0;
        double prev = row[lo];
        for (uint32_t i = lo; i < n; i++) {
          double v = row[i];
          if (isnan(v)) continue;
          double d = v - prev;
          if (d < 0.0) {
            if ((-d * 8.0) < prev) corr += prev - v;
            else corr += prev;
          }
          prev = v;
          row[i] = v + corr;
        }
        break;
      }
      default:
        break;
    }
  }
}

extern "C" {

int vmgpu_transform(int32_t func, double* values, uint32_t n_series,
                    uint32_t n_grid, const int64_t* ts, const double* arg1,
                    const double* arg2, double scalar_arg,
                    uint8_t* keep_flags, char* errbuf, size_t errbuf_len) {
  if (!values || n_series == 0 || n_grid == 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad transform args");
  hipStream_t st = 0;
  size_t vbytes = (size_t)n_series * n_grid * 8;
  VmDevBuf dv, dts, da1, da2, dscr, dkeep;
  VM_HIP_TRY(dv.alloc(vbytes), "alloc tf values");
  VM_HIP_TRY(hipMemcpyAsync(dv.p, values, vbytes, hipMemcpyHostToDevice, st), "ul tf");
  const int64_t* d_ts = nullptr;
  const double* d_a1 = nullptr;
  const double* d_a2 = nullptr;
  if (ts) {
    VM_HIP_TRY(dts.alloc((size_t)n_grid * 8), "alloc tf ts");
    VM_HIP_TRY(hipMemcpyAsync(dts.p, ts, (size_t)n_grid * 8, hipMemcpyHostToDevice, st), "ul tf ts");
    d_ts = (const int64_t*)dts.p;
  }
  if (arg1) {
    VM_HIP_TRY(da1.alloc((size_t)n_grid * 8), "alloc tf a1");
    VM_HIP_TRY(hipMemcpyAsync(da1.p, arg1, (size_t)n_grid * 8, hipMemcpyHostToDevice, st), "ul tf a1");
    d_a1 = (const double*)da1.p;
  }
  if (arg2) {
    VM_HIP_TRY(da2.alloc((size_t)n_grid * 8), "alloc tf a2");
    VM_HIP_TRY(hipMemcpyAsync(da2.p, arg2, (size_t)n_grid * 8, hipMemcpyHostToDevice, st), "ul tf a2");
    d_a2 = (const double*)da2.p;
  }
  bool elementwise = func < VMGPU_TF_SERIES_BASE;
  if (elementwise) {
    uint64_t total = (uint64_t)n_series * n_grid;
    uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(transform_elementwise_kernel, dim3(blocks), dim3(256),
                       0, st, func, (double*)dv.p, (uint64_t)n_series, n_grid,
                       d_a1, d_a2);
  } else {
    bool needs_scratch = (func == VMGPU_TF_RANGE_MAD ||
                          func == VMGPU_TF_RANGE_TRIM_OUTLIERS ||
                          func == VMGPU_TF_RANGE_TRIM_SPIKES ||
                          func == VMGPU_TF_RANGE_QUANTILE);
    double* d_scr = nullptr;
    if (needs_scratch) {
      VM_HIP_TRY(dscr.alloc(vbytes), "alloc tf scratch");
      d_scr = (double*)dscr.p;
    }
    uint8_t* d_keep = nullptr;
    if (keep_flags) {
      VM_HIP_TRY(dkeep.alloc(n_series), "alloc tf keep");
      d_keep = (uint8_t*)dkeep.p;
    }
    uint32_t blocks = std::min<uint32_t>((n_series + 255) / 256, 4096);
    hipLaunchKernelGGL(transform_series_kernel, dim3(blocks), dim3(256), 0, st,
                       func, (double*)dv.p, (uint64_t)n_series, n_grid, d_ts,
                       d_a1, scalar_arg, d_scr, d_keep);
    if (keep_flags)
      VM_HIP_TRY(hipMemcpyAsync(keep_flags, dkeep.p, n_series,
                              hipMemcpyDeviceToHost, st), "dl tf keep");
  }
  VM_HIP_TRY(hipMemcpyAsync(values, dv.p, vbytes, hipMemcpyDeviceToHost, st), "dl tf");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync tf");
  hipError_t kerr = hipGetLastError();
  if (kerr != hipSuccess) return vm_hip_err(errbuf, errbuf_len, "tf kernel", kerr);
  return 0;
}

}  /* extern "C" */
