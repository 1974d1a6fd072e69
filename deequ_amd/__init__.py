"""deequ_amd -- MI355X-native backend for deequ's metric-computation hot path.

The public names mirror the reference's Scala API (`com.amazon.deequ.analyzers`,
`...analyzers.runners`): analyzers, states, `AnalysisRunner`, `AnalyzerContext`.  All compute
goes through the C-ABI library `libdeequ_amd.so` (hand-written gfx950 HIP kernels); there is
no CPU fallback.
"""
from .analyzers import (Analyzer, ApproxCountDistinct, ApproxQuantile, ApproxQuantiles, Completeness, Compliance, CountDistinct, DataType,
                        DataTypeInstances,
                        Distinctness, Entropy, FrequencyBasedAnalyzer, GroupingAnalyzer, Histogram,
                        KLLParameters, KLLSketch,
                        Correlation, MaxLength, Maximum, Mean, MinLength, Minimum, MutualInformation,
                        PatternMatch, Preconditions,
                        ScanShareableAnalyzer, ScanShareableFrequencyBasedAnalyzer, Size,
                        StandardDeviation, StandardScanShareableAnalyzer, Sum, Uniqueness,
                        UniqueValueRatio)
from .frequencies import FrequenciesAndNumRows, FrequencyTable
from .distance import Distance
from .engine import Plan, current_device, run_scan, set_device
from .metrics import (BucketDistribution, BucketValue, KLLMetric, Distribution, DistributionValue, DoubleMetric, EmptyStateException, Entity,
                      Failure, HistogramMetric, KeyedDoubleMetric,
                      IllegalAnalyzerParameterException, MetricCalculationException,
                      MetricCalculationRuntimeException, NoSuchColumnException, Success,
                      WrongColumnTypeException)
from .runner import (Analysis, AnalysisRunBuilder, AnalysisRunner, AnalyzerContext,
                     InMemoryStateProvider)
from .states import (ApproxCountDistinctState, CorrelationState, DataTypeHistogram, MaxState, MeanState, MinState,
                     NumMatches,
                     NumMatchesAndCount, StandardDeviationState, State, SumState,
                     KLLState, NonSampleCompactor, QuantileNonSample,
                     ApproxQuantileState, PercentileDigest)
from .state_provider import HdfsStateProvider
from . import kll
from . import quantiles
from .arrow import ArrowBatch, ArrowTable
from .table import Column, PartitionedTable, Table
from .rowlevel import RowLevelResults, row_level_results
from .comparison import MatchCounts, MatchResult, dataset_match, referential_integrity
from .take import take
from .correlation import CorrelationMatrix, correlation_matrix
from .schema import RowLevelSchema, RowLevelSchemaValidationResult, RowLevelSchemaValidator

__all__ = [n for n in dir() if not n.startswith("_")]
