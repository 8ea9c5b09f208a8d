from revisit_bpr.modules.neg_samplers import AdaptiveSampler, DynamicSampler, Sampler, UniformSampler

__all__ = ["Sampler", "UniformSampler", "AdaptiveSampler", "DynamicSampler"]
