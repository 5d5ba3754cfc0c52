function pathLoss = config5GNRModels(pathLossConfig, carrierFreq, losCondition, bsPosition, uePosition)
%CONFIG5GNRMODELS  Drop-in replacement body for +communication/+pathlossModels/config5GNRModels.m: TR 38.901 7.4.1 path loss [dB] of the
%   scenario named by pathLossConfig ('UMa' 'UMi' 'RMa' 'InH' 'InF-SL' 'InF-DL' 'InF-SH' 'InF-DH' 'InF-HH'), 0 for equal positions.  The third
%   coordinate of the FIRST position is taken as h_BS, of the second as h_UT, whatever the caller passes (INTEGRATION.md, applyChannelModel recipe).
    pathLoss = isac_mex('pathLoss', char(pathLossConfig), double(carrierFreq), double(losCondition), double(bsPosition(:)).', double(uePosition(:)).');
end
