"""EDM constants of MonsterDiffusion (Karras et al., arXiv 2206.00364: the training distribution of ln sigma, the rho schedule between
sigma_min and sigma_max, and the stochastic sampler's churn window of table 5, ImageNet-64 row)."""
P_mean, P_std = -1.2, 1.2
sigma_data = 0.5
rho = 7
sigma_min, sigma_max = 1e-2, 80
S_tmin, S_tmax = 0.05, 50
S_churn = 80
S_noise = 1.003
